// SSIM of two fp32 channel-last images [H, W, C] (Wang et al. 2004), forward and backward -- the image metric of nerf2mesh_amd/metrics.py and the
// structural term of stage 1 (lambda_ssim).  The reference carries the metric as a commented-out meter (nerf/utils.py:351-465) whose call is
// torchmetrics' structural_similarity_index_measure at its defaults; this follows those defaults except for the border rule.
//
//   window   11 x 11 Gaussian, sigma 1.5, separable; the 11 taps come from the host (float64, normalised, rounded to fp32): no device exp
//   border   VALID windows only, no padding: the map is [H - 10, W - 10, C]
//   moments  mu_x, mu_y, E[x^2], E[y^2], E[xy] per window and channel; s_x^2 = E[x^2] - mu_x^2, s_y^2, s_xy likewise
//   S        (2 mu_x mu_y + C1) (2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1) (s_x^2 + s_y^2 + C2)),  C1 = 0.01^2, C2 = 0.03^2;  ssim = mean S
//
// A row of a channel-last image is W * C floats in which the horizontal neighbours of one channel lie C floats apart, so both kernels work
// in FLAT columns f = x * C + c: a tile of 32 x 16 pixels is kTX * C flat columns wide, its halo 10 * C more, and no lane ever needs to know
// which channel it holds.  Consecutive lanes take consecutive flat columns: global loads are coalesced and LDS rows are read conflict-free.
//
// forward, one workgroup (256 threads) per tile of 32 x 16 windows:
//   1. x and y of the tile's 42 x 26 pixels -> LDS (zero past the image: such taps only feed windows that are not written);
//   2. horizontal pass: the five quantities for 26 rows x 32 * C flat columns -> LDS;
//   3. vertical pass, S, the optional map and the three optional derivative maps; the workgroup's sum of S -> partials[block], lanes, waves
//      in a fixed order.  ssim_mean_kernel (one workgroup) then sums the partials in a fixed order: no float atomics anywhere.
//   LDS for C = 3: 2 * 26 * 128 + 5 * 26 * 96 floats = 76.5 KiB, two workgroups per CU (160 KiB); C = 1: 29.5 KiB.
//
// backward: with the moments m1 = mu_x, m2 = E[x^2], m3 = E[xy] (y is a constant: no gradient),
//   dS/dm2 = -S / b2,  dS/dm3 = 2 a1 / (b1 b2),  dS/dm1 = 2 mu_y (a2 - a1) / (b1 b2) + 2 mu_x S (1 / b2 - 1 / b1)
//   (a1, a2 the numerator's factors, b1, b2 the denominator's; s_x^2 and s_xy carry m1 along), and since every moment is linear in x, x^2, xy
//   grad_x[p] = g / n * sum over windows q that contain p of w(p - q) (A[q] + 2 x[p] B[q] + y[p] Cq[q])
// -- the three derivative maps filtered with the transposed ("full") window: the same two passes over a tile of 32 x 16 PIXELS whose halo
// is the 10 map rows / columns before it (zero outside the map).  A gather: every pixel is written once, the same bits on every run.
// Entry points are declared in include/n2m_hip.h.
#include "n2m_common.hpp"

namespace {

constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kTX = 32, kTY = 16;                 // tile: windows (forward) / pixels (backward)
constexpr int kRows = kTY + kHalo;                // 26 staged rows
constexpr int kThreads = 256;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

template <int C> struct Tile {
    static constexpr int kOutW = kTX * C;                         // flat columns of the tile
    static constexpr int kInW = (kTX + kHalo) * C;                // ... with the halo
    static constexpr int kInStride = (kInW + 31) / 32 * 32 + (C == 1 ? 1 : 0);   // 128 (C = 3) / 65 (C = 1): two rows of one wave never share a bank
};

struct Taps { float w[kWin]; };

// dS[0], dS[1], dS[2] = dS/dmu_x, dS/dE[x^2], dS/dE[xy]: three planes of the map's size
template <int C>
__global__ void __launch_bounds__(kThreads, 2)
ssim_forward_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, Taps taps, float* __restrict__ smap,
                    float* __restrict__ dS, float* __restrict__ partials) {
    using T = Tile<C>;
    __shared__ float in_x[kRows * T::kInStride], in_y[kRows * T::kInStride];
    __shared__ float hp[5][kRows * T::kOutW];
    __shared__ float red[kThreads / N2M_WAVE];
    const int Hm = H - kHalo, Wm = W - kHalo;                     // the map's extent
    const int row0 = blockIdx.y * kTY, col0 = blockIdx.x * kTX;   // the tile's first window = its first pixel
    const int rowlen = W * C;
    const int tid = threadIdx.x;

    for (int i = tid; i < kRows * T::kInW; i += kThreads) {
        const int r = i / T::kInW, f = i - r * T::kInW;
        const int gr = row0 + r, gf = col0 * C + f;
        const bool in = gr < H && gf < rowlen;
        const size_t g = (size_t)gr * rowlen + gf;
        in_x[r * T::kInStride + f] = in ? x[g] : 0.0f;
        in_y[r * T::kInStride + f] = in ? y[g] : 0.0f;
    }
    __syncthreads();

    for (int i = tid; i < kRows * T::kOutW; i += kThreads) {
        const int r = i / T::kOutW, f = i - r * T::kOutW;
        const float* px = in_x + r * T::kInStride + f;
        const float* py = in_y + r * T::kInStride + f;
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float a = px[k * C], b = py[k * C], w = taps.w[k];
            mx = fmaf(w, a, mx);
            my = fmaf(w, b, my);
            xx = fmaf(w, a * a, xx);
            yy = fmaf(w, b * b, yy);
            xy = fmaf(w, a * b, xy);
        }
        hp[0][i] = mx; hp[1][i] = my; hp[2][i] = xx; hp[3][i] = yy; hp[4][i] = xy;
    }
    __syncthreads();

    const size_t plane = (size_t)Hm * Wm * C;
    float sum = 0.0f;
    for (int i = tid; i < kTY * T::kOutW; i += kThreads) {        // kTY * kOutW is a multiple of 256: every lane makes every trip
        const int r = i / T::kOutW, f = i - r * T::kOutW;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hp[q][(r + k) * T::kOutW + f], m[q]);
        }
        const float mx = m[0], my = m[1];
        const float sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
        const float a1 = 2.0f * mx * my + kC1, a2 = 2.0f * sxy + kC2;
        const float b1 = mx * mx + my * my + kC1, b2 = sxx + syy + kC2;
        const float S = (a1 * a2) / (b1 * b2);
        const int gr = row0 + r, gf = col0 * C + f;
        const bool live = gr < Hm && gf < Wm * C;
        sum += live ? S : 0.0f;
        if (live) {
            const size_t o = (size_t)gr * (Wm * C) + gf;
            if (smap) smap[o] = S;
            if (dS) {
                const float ib1 = 1.0f / b1, ib2 = 1.0f / b2;
                dS[o] = 2.0f * my * (a2 - a1) * (ib1 * ib2) + 2.0f * mx * S * (ib2 - ib1);
                dS[plane + o] = -S * ib2;
                dS[2 * plane + o] = 2.0f * a1 * (ib1 * ib2);
            }
        }
    }
    const float ws = n2m_wave_sum(sum);                            // all 64 lanes active: the loop above is uniform and `live` is a select
    if ((tid & (N2M_WAVE - 1)) == 0) red[tid / N2M_WAVE] = ws;
    __syncthreads();
    if (tid == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = (sum of the partials) / n: strided per-lane sums, wave sums, the four waves -- one order, whatever the machine does
__global__ void __launch_bounds__(kThreads)
ssim_mean_kernel(const float* __restrict__ partials, uint32_t count, float inv_n, float* __restrict__ out) {
    __shared__ float red[kThreads / N2M_WAVE];
    float s = 0.0f;
    for (uint32_t i = threadIdx.x; i < count; i += kThreads) s += partials[i];
    const float ws = n2m_wave_sum(s);
    if ((threadIdx.x & (N2M_WAVE - 1)) == 0) red[threadIdx.x / N2M_WAVE] = ws;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}

template <int C>
__global__ void __launch_bounds__(kThreads, 2)
ssim_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dS, int H, int W, Taps taps,
                     const float* __restrict__ g, float inv_n, float* __restrict__ grad_x) {
    using T = Tile<C>;
    __shared__ float in_d[3][kRows * T::kInStride];
    __shared__ float hp[3][kRows * T::kOutW];
    const int Hm = H - kHalo, Wm = W - kHalo;
    const int row0 = blockIdx.y * kTY, col0 = blockIdx.x * kTX;   // the tile's first pixel; staged map rows / columns begin kHalo before it
    const int maplen = Wm * C;
    const size_t plane = (size_t)Hm * maplen;
    const int tid = threadIdx.x;

    for (int i = tid; i < kRows * T::kInW; i += kThreads) {
        const int r = i / T::kInW, f = i - r * T::kInW;
        const int gr = row0 - kHalo + r, gf = (col0 - kHalo) * C + f;
        const bool in = gr >= 0 && gr < Hm && gf >= 0 && gf < maplen;
        const size_t o = in ? (size_t)gr * maplen + gf : 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) in_d[q][r * T::kInStride + f] = in ? dS[q * plane + o] : 0.0f;
    }
    __syncthreads();

    // pixel column px takes window columns px - 10 .. px with taps 10 .. 0: staged flat column f + (10 - k) * C carries tap k
    for (int i = tid; i < kRows * T::kOutW; i += kThreads) {
        const int r = i / T::kOutW, f = i - r * T::kOutW;
        float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 3; ++q) m[q] = fmaf(w, in_d[q][r * T::kInStride + f + (kHalo - k) * C], m[q]);
        }
        hp[0][i] = m[0]; hp[1][i] = m[1]; hp[2][i] = m[2];
    }
    __syncthreads();

    const float scale = g[0] * inv_n;
    const int rowlen = W * C;
    for (int i = tid; i < kTY * T::kOutW; i += kThreads) {
        const int r = i / T::kOutW, f = i - r * T::kOutW;
        const int gr = row0 + r, gf = col0 * C + f;
        if (gr >= H || gf >= rowlen) continue;
        float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 3; ++q) m[q] = fmaf(w, hp[q][(r + kHalo - k) * T::kOutW + f], m[q]);
        }
        const size_t o = (size_t)gr * rowlen + gf;
        grad_x[o] = scale * (m[0] + 2.0f * x[o] * m[1] + y[o] * m[2]);
    }
}

// ------------------------------------------------------------------------------------------------ batched square patches [B, P, P, C]
// The stage-0 patch term (trainer.Stage0Trainer, lambda_patch_ssim): B patches of P x P pixels, 11 <= P <= 64, the definition above per patch.
// The frame kernels would take one launch pair per patch and fill 36 of a workgroup's 512 window slots at P = 16, so the workgroup here is
// sized by the PATCH: it stages whole pixel rows of one patch (a patch is contiguous, so staging is a straight coalesced copy, LDS index =
// offset in the patch), works in the same flat columns f = x * C + c, and takes a BAND of rows of that patch:
//   forward    a band of R window rows stages R + 10 pixel rows of x and y and the five horizontally filtered planes of those rows
//   backward   a band of R pixel rows stages the R + 10 map rows before it, 10 zero columns on either side, and three filtered planes
// Three tiers by P, each with static LDS sized for its largest patch (C = 3 bytes; 160 KiB per CU):
//   P <= 16   forward  whole patch (<= 6 window rows), 16 rows:   6.0 + 5.6 KiB = 11.6 KiB   backward R = 16 (whole), 26 rows: 23.8 + 14.6 = 38.4 KiB
//   P <= 32   forward  whole patch (<= 22 window rows), 32 rows: 24.0 + 41.3 = 65.3 KiB       backward R = 16 (two bands), 26 rows: 38.4 + 29.3 = 67.6 KiB
//   P <= 64   forward  R = 6 (<= 9 bands), 16 rows:              24.0 + 50.6 = 74.6 KiB       backward R = 6 (<= 11 bands), 16 rows: 41.6 + 36.0 = 77.6 KiB
// so at least two workgroups fit a CU by LDS in every tier (P = 64 whole would need over 300 KiB).  The per-window arithmetic is the frame
// kernel's, statement for statement.  Sums: lanes stride the band's windows, wave sums, the four waves -> partials[b * nbands + band];
// ssim_patches_mean_kernel adds a patch's bands in band order (per_patch[b]) and the patches in a fixed strided order (out[0]): no float
// atomics, the same bits on every run, and nothing of patch b depends on another patch.
struct PatchTier { int max_p, fwd_rows, fwd_band, bwd_rows, bwd_band; };
constexpr PatchTier kTier16{16, 16, 6, 26, 16}, kTier32{32, 32, 22, 26, 16}, kTier64{64, 16, 6, 16, 6};
constexpr int kPatchMin = kWin, kPatchMax = 64;

template <int C, int kMaxP, int kMaxRows>
__global__ void __launch_bounds__(kThreads, 2)
ssim_patches_forward_kernel(const float* __restrict__ x, const float* __restrict__ y, int P, int R, int nbands, Taps taps,
                            float* __restrict__ dS, float* __restrict__ partials) {
    __shared__ float in_x[kMaxRows * kMaxP * C], in_y[kMaxRows * kMaxP * C];
    __shared__ float hp[5][kMaxRows * (kMaxP - kHalo) * C];
    __shared__ float red[kThreads / N2M_WAVE];
    const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
    const int Pm = P - kHalo, inW = P * C, outW = Pm * C;          // the map's extent; flat row lengths of the patch and of the map
    const int wrow0 = band * R;                                    // the band's first window row = its first staged pixel row
    const int wrows = min(R, Pm - wrow0), rows = wrows + kHalo;    // rows <= kMaxRows and wrow0 + rows <= P (host: R + 10 <= kMaxRows)
    const int tid = threadIdx.x;

    const size_t pbase = ((size_t)b * P + wrow0) * inW;
    for (int i = tid; i < rows * inW; i += kThreads) {
        in_x[i] = x[pbase + i];
        in_y[i] = y[pbase + i];
    }
    __syncthreads();

    for (int i = tid; i < rows * outW; i += kThreads) {
        const int r = i / outW, f = i - r * outW;
        const float* px = in_x + r * inW + f;
        const float* py = in_y + r * inW + f;
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float a = px[k * C], b2 = py[k * C], w = taps.w[k];
            mx = fmaf(w, a, mx);
            my = fmaf(w, b2, my);
            xx = fmaf(w, a * a, xx);
            yy = fmaf(w, b2 * b2, yy);
            xy = fmaf(w, a * b2, xy);
        }
        hp[0][i] = mx; hp[1][i] = my; hp[2][i] = xx; hp[3][i] = yy; hp[4][i] = xy;
    }
    __syncthreads();

    const size_t plane = (size_t)Pm * outW;
    float* __restrict__ dSb = dS ? dS + (size_t)b * 3 * plane : nullptr;
    const int n = wrows * outW;
    float sum = 0.0f;
    for (int i0 = 0; i0 < n; i0 += kThreads) {                     // uniform trip count: the wave sum below needs all 64 lanes
        const int i = i0 + tid;
        float S = 0.0f;
        if (i < n) {
            const int r = i / outW, f = i - r * outW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float w = taps.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hp[q][(r + k) * outW + f], m[q]);
            }
            const float mx = m[0], my = m[1];
            const float sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
            const float a1 = 2.0f * mx * my + kC1, a2 = 2.0f * sxy + kC2;
            const float b1 = mx * mx + my * my + kC1, b2 = sxx + syy + kC2;
            S = (a1 * a2) / (b1 * b2);
            if (dSb) {
                const size_t o = (size_t)(wrow0 + r) * outW + f;
                const float ib1 = 1.0f / b1, ib2 = 1.0f / b2;
                dSb[o] = 2.0f * my * (a2 - a1) * (ib1 * ib2) + 2.0f * mx * S * (ib2 - ib1);
                dSb[plane + o] = -S * ib2;
                dSb[2 * plane + o] = 2.0f * a1 * (ib1 * ib2);
            }
        }
        sum += S;
    }
    const float ws = n2m_wave_sum(sum);
    if ((tid & (N2M_WAVE - 1)) == 0) red[tid / N2M_WAVE] = ws;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// per_patch[b] = (the patch's band sums, in band order) / n_patch; out[0] = (the patch sums: strided per lane, wave sums, the four waves) / n_all
__global__ void __launch_bounds__(kThreads)
ssim_patches_mean_kernel(const float* __restrict__ partials, uint32_t B, uint32_t nbands, float inv_patch, float inv_all,
                         float* __restrict__ per_patch, float* __restrict__ out) {
    __shared__ float red[kThreads / N2M_WAVE];
    float s = 0.0f;
    for (uint32_t b = threadIdx.x; b < B; b += kThreads) {
        float p = 0.0f;
        for (uint32_t k = 0; k < nbands; ++k) p += partials[(size_t)b * nbands + k];
        per_patch[b] = p * inv_patch;
        s += p;
    }
    const float ws = n2m_wave_sum(s);
    if ((threadIdx.x & (N2M_WAVE - 1)) == 0) red[threadIdx.x / N2M_WAVE] = ws;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_all;
}

template <int C, int kMaxP, int kMaxRows>
__global__ void __launch_bounds__(kThreads, 2)
ssim_patches_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dS, int P, int R, int nbands,
                             Taps taps, const float* __restrict__ g, float inv_n, float* __restrict__ grad_x) {
    __shared__ float in_d[3][kMaxRows * (kMaxP + kHalo) * C];
    __shared__ float hp[3][kMaxRows * kMaxP * C];
    const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
    const int Pm = P - kHalo, maplen = Pm * C;
    const int inW = (P + kHalo) * C, outW = P * C;                 // staged map row: 10 zero columns, the map's, 10 zero columns; pixel row
    const int prow0 = band * R;                                    // the band's first pixel row; staged map rows begin kHalo before it
    const int prows = min(R, P - prow0), rows = prows + kHalo;     // rows <= kMaxRows (host: R + 10 <= kMaxRows)
    const size_t plane = (size_t)Pm * maplen;
    const float* __restrict__ dSb = dS + (size_t)b * 3 * plane;
    const int tid = threadIdx.x;

    for (int i = tid; i < rows * inW; i += kThreads) {
        const int r = i / inW, f = i - r * inW;
        const int gr = prow0 - kHalo + r, gf = f - kHalo * C;
        const bool in = gr >= 0 && gr < Pm && gf >= 0 && gf < maplen;
        const size_t o = in ? (size_t)gr * maplen + gf : 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) in_d[q][i] = in ? dSb[q * plane + o] : 0.0f;
    }
    __syncthreads();

    for (int i = tid; i < rows * outW; i += kThreads) {
        const int r = i / outW, f = i - r * outW;
        float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 3; ++q) m[q] = fmaf(w, in_d[q][r * inW + f + (kHalo - k) * C], m[q]);
        }
        hp[0][i] = m[0]; hp[1][i] = m[1]; hp[2][i] = m[2];
    }
    __syncthreads();

    const float scale = g[0] * inv_n;
    const size_t pbase = ((size_t)b * P + prow0) * outW;
    for (int i = tid; i < prows * outW; i += kThreads) {
        const int r = i / outW, f = i - r * outW;
        float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 3; ++q) m[q] = fmaf(w, hp[q][(r + kHalo - k) * outW + f], m[q]);
        }
        const size_t o = pbase + i;
        grad_x[o] = scale * (m[0] + 2.0f * x[o] * m[1] + y[o] * m[2]);
    }
}

const PatchTier& patch_tier(uint32_t P) { return P <= 16 ? kTier16 : P <= 32 ? kTier32 : kTier64; }

int check_patches(const char* who, uint32_t B, uint32_t P, uint32_t C) {
    N2M_REQUIRE(P >= (uint32_t)kPatchMin && P <= (uint32_t)kPatchMax, N2M_EINVAL, "%s: P must be 11 .. 64 (one valid 11 x 11 window; the largest staged patch), got %u", who, P);
    N2M_REQUIRE(C == 1 || C == 3, N2M_EINVAL, "%s: C must be 1 or 3, got %u", who, C);
    N2M_REQUIRE(B >= 1 && B <= (1u << 20), N2M_EINVAL, "%s: B must be 1 .. 2^20 patches, got %u", who, B);
    return 0;
}

int check_shape(const char* who, uint32_t H, uint32_t W, uint32_t C) {
    N2M_REQUIRE(H >= (uint32_t)kWin && W >= (uint32_t)kWin, N2M_EINVAL, "%s: H and W must be at least 11 (one valid 11 x 11 window), got %u x %u", who, H, W);
    N2M_REQUIRE(C == 1 || C == 3, N2M_EINVAL, "%s: C must be 1 or 3, got %u", who, C);
    N2M_REQUIRE((uint64_t)H * W * C < (1ull << 31) && H <= 0xFFFFu * (uint32_t)kTY, N2M_EINVAL, "%s: image too large (%u x %u x %u)", who, H, W, C);
    return 0;
}

Taps load_taps(const float* taps_host) {
    Taps t;
    for (int k = 0; k < kWin; ++k) t.w[k] = taps_host[k];
    return t;
}

}  // namespace

extern "C" uint32_t n2m_ssim_partials(uint32_t H, uint32_t W) {
    if (H < (uint32_t)kWin || W < (uint32_t)kWin) return 0;
    return n2m_ceil_div(W - kHalo, kTX) * n2m_ceil_div(H - kHalo, kTY);
}

extern "C" int n2m_ssim_forward(const float* x, const float* y, uint32_t H, uint32_t W, uint32_t C, const float* taps_host, float* map_or_null,
                                float* dS_or_null, float* partials, float* out, void* stream) {
    if (int rc = check_shape("ssim_forward", H, W, C)) return rc;
    N2M_REQUIRE(x && y && taps_host && partials && out, N2M_ENULL, "ssim_forward: NULL tensor (x, y, taps, partials and out are required)");
    const dim3 grid(n2m_ceil_div(W - kHalo, kTX), n2m_ceil_div(H - kHalo, kTY));
    const Taps t = load_taps(taps_host);
    hipStream_t s = (hipStream_t)stream;
    if (C == 3) ssim_forward_kernel<3><<<grid, kThreads, 0, s>>>(x, y, (int)H, (int)W, t, map_or_null, dS_or_null, partials);
    else ssim_forward_kernel<1><<<grid, kThreads, 0, s>>>(x, y, (int)H, (int)W, t, map_or_null, dS_or_null, partials);
    N2M_CHECK_LAUNCH();
    const double n = (double)(H - kHalo) * (double)(W - kHalo) * (double)C;
    ssim_mean_kernel<<<1, kThreads, 0, s>>>(partials, grid.x * grid.y, (float)(1.0 / n), out);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" uint32_t n2m_ssim_patches_partials(uint32_t B, uint32_t P) {
    if (P < (uint32_t)kPatchMin || P > (uint32_t)kPatchMax) return 0;
    return B * n2m_ceil_div(P - kHalo, patch_tier(P).fwd_band);
}

extern "C" int n2m_ssim_patches_forward(const float* x, const float* y, uint32_t B, uint32_t P, uint32_t C, const float* taps_host,
                                        float* dS_or_null, float* partials, float* per_patch, float* out, void* stream) {
    if (int rc = check_patches("ssim_patches_forward", B, P, C)) return rc;
    N2M_REQUIRE(x && y && taps_host && partials && per_patch && out, N2M_ENULL,
                "ssim_patches_forward: NULL tensor (x, y, taps, partials, per_patch and out are required)");
    const PatchTier& t = patch_tier(P);
    const int R = t.fwd_band, nbands = (int)n2m_ceil_div(P - kHalo, R);
    const uint32_t grid = B * (uint32_t)nbands;
    const Taps taps = load_taps(taps_host);
    hipStream_t s = (hipStream_t)stream;
#define N2M_SSIM_PATCHES_FWD(CC, T) \
    ssim_patches_forward_kernel<CC, T.max_p, T.fwd_rows><<<grid, kThreads, 0, s>>>(x, y, (int)P, R, nbands, taps, dS_or_null, partials)
    if (C == 3) {
        if (P <= 16) N2M_SSIM_PATCHES_FWD(3, kTier16); else if (P <= 32) N2M_SSIM_PATCHES_FWD(3, kTier32); else N2M_SSIM_PATCHES_FWD(3, kTier64);
    } else {
        if (P <= 16) N2M_SSIM_PATCHES_FWD(1, kTier16); else if (P <= 32) N2M_SSIM_PATCHES_FWD(1, kTier32); else N2M_SSIM_PATCHES_FWD(1, kTier64);
    }
#undef N2M_SSIM_PATCHES_FWD
    N2M_CHECK_LAUNCH();
    const double n_patch = (double)(P - kHalo) * (double)(P - kHalo) * (double)C;
    ssim_patches_mean_kernel<<<1, kThreads, 0, s>>>(partials, B, (uint32_t)nbands, (float)(1.0 / n_patch), (float)(1.0 / (n_patch * (double)B)),
                                                    per_patch, out);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_ssim_patches_backward(const float* x, const float* y, const float* dS, uint32_t B, uint32_t P, uint32_t C,
                                         const float* taps_host, const float* g, float* grad_x, void* stream) {
    if (int rc = check_patches("ssim_patches_backward", B, P, C)) return rc;
    N2M_REQUIRE(x && y && dS && taps_host && g && grad_x, N2M_ENULL, "ssim_patches_backward: NULL tensor");
    const PatchTier& t = patch_tier(P);
    const int R = t.bwd_band, nbands = (int)n2m_ceil_div(P, R);
    const uint32_t grid = B * (uint32_t)nbands;
    const Taps taps = load_taps(taps_host);
    const float inv_n = (float)(1.0 / ((double)(P - kHalo) * (double)(P - kHalo) * (double)C * (double)B));
    hipStream_t s = (hipStream_t)stream;
#define N2M_SSIM_PATCHES_BWD(CC, T) \
    ssim_patches_backward_kernel<CC, T.max_p, T.bwd_rows><<<grid, kThreads, 0, s>>>(x, y, dS, (int)P, R, nbands, taps, g, inv_n, grad_x)
    if (C == 3) {
        if (P <= 16) N2M_SSIM_PATCHES_BWD(3, kTier16); else if (P <= 32) N2M_SSIM_PATCHES_BWD(3, kTier32); else N2M_SSIM_PATCHES_BWD(3, kTier64);
    } else {
        if (P <= 16) N2M_SSIM_PATCHES_BWD(1, kTier16); else if (P <= 32) N2M_SSIM_PATCHES_BWD(1, kTier32); else N2M_SSIM_PATCHES_BWD(1, kTier64);
    }
#undef N2M_SSIM_PATCHES_BWD
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_ssim_backward(const float* x, const float* y, const float* dS, uint32_t H, uint32_t W, uint32_t C, const float* taps_host,
                                 const float* g, float* grad_x, void* stream) {
    if (int rc = check_shape("ssim_backward", H, W, C)) return rc;
    N2M_REQUIRE(x && y && dS && taps_host && g && grad_x, N2M_ENULL, "ssim_backward: NULL tensor");
    const dim3 grid(n2m_ceil_div(W, kTX), n2m_ceil_div(H, kTY));
    const Taps t = load_taps(taps_host);
    const double n = (double)(H - kHalo) * (double)(W - kHalo) * (double)C;
    hipStream_t s = (hipStream_t)stream;
    if (C == 3) ssim_backward_kernel<3><<<grid, kThreads, 0, s>>>(x, y, dS, (int)H, (int)W, t, g, (float)(1.0 / n), grad_x);
    else ssim_backward_kernel<1><<<grid, kThreads, 0, s>>>(x, y, dS, (int)H, (int)W, t, g, (float)(1.0 / n), grad_x);
    N2M_CHECK_LAUNCH();
    return 0;
}
