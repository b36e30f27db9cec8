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
