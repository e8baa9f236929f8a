// Modulated deformable convolution (DCNv2; models/backbones/deformable/ of the reference, source/cpu/dcn.im2col.cpp
// :156-190): the sampling half, on NHWC activations.  3x3 taps k = 3i + j, stride 1, pad 1, dilation 1, G deformable
// groups of Cg = C/G channels.  For output pixel (h, w), tap k, group g, with om (N,H,W,P), P >= 27G:
//   dh = om[18g + 2k], dw = om[18g + 2k + 1], m = om[18G + 9g + k]  (sigmoid(.) of it when the channel holds a logit)
//   sample point (h - 1 + i + dh, w - 1 + j + dw); a bilinear corner outside [0,H-1] x [0,W-1] contributes 0
//   forward   cols[pix][k*C + c] = m * sum_corners weight * x[corner][c]      (fp32 blend, one rounding)
//   backward  dom  = gradients towards dh, dw and the mask channel (written; pad channels 0)
//             dx32 += dcol * m * weight at every corner with a non-zero weight  (fp32 atomics)
// The convolution itself is the 1x1 gather-GEMM over cols with Ci = 9C: column k*C + c is the K order of pack mode 0
// of the (Co,C,3,3) weight.
// Forward: an HBM stream; one thread owns one 16-byte channel chunk of one (pixel, tap), issues its four corner
// vectors before it uses any of them, and a grid of resident workgroups strides over the chunks.  No LDS, no atomics.
// Backward: L = min(64, Cg rounded up to a power of two) lanes own one (pixel, tap, group) and run along its channels,
// so one atomic wave-instruction adds 64 contiguous floats (Cg >= 64) or 64/L segments of neighbouring groups.  The
// three channel sums of an item run lane by lane in channel order, then an xor butterfly over the L lanes: a fixed
// order, so dom is the same bits from call to call.  dx32 depends on the atomics' arrival order in its last bits.
#include <algorithm>

#include "scd_common.h"

namespace {
SCD_KERNEL_NS_BEGIN

// The sample point of (output pixel (h, w), tap k) and its bilinear corners q = 2a + b at (h0 + a, w0 + b)
struct DcnSample {
    int h0, w0;
    float lh, lw;       // fractional parts
    float wt[4];        // corner weights (1-lh)(1-lw), (1-lh)lw, lh(1-lw), lh*lw
    bool ok[4];         // corner inside the image
};

__device__ __forceinline__ DcnSample dcn_sample(int h, int w, int k, float dh, float dw, int H, int W) {
    const int i = k / 3, j = k - 3 * i;
    // a point a pixel or more outside has no corner inside wherever it lies: clamped to [-2, extent + 1] it keeps
    // that property and the float -> int conversion is defined for every offset (fminf / fmaxf drop a NaN)
    const float ph = fminf(fmaxf((float)(h - 1 + i) + dh, -2.0f), (float)H + 1.0f);
    const float pw = fminf(fmaxf((float)(w - 1 + j) + dw, -2.0f), (float)W + 1.0f);
    const float fh = floorf(ph), fw = floorf(pw);
    DcnSample s;
    s.h0 = (int)fh;
    s.w0 = (int)fw;
    s.lh = ph - fh;
    s.lw = pw - fw;
    s.wt[0] = (1.0f - s.lh) * (1.0f - s.lw);
    s.wt[1] = (1.0f - s.lh) * s.lw;
    s.wt[2] = s.lh * (1.0f - s.lw);
    s.wt[3] = s.lh * s.lw;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int hi = s.h0 + (q >> 1), wi = s.w0 + (q & 1);
        s.ok[q] = hi >= 0 && hi < H && wi >= 0 && wi < W;
    }
    return s;
}

// element offset of channel 0 of corner q of image n (only for a corner that is inside)
__device__ __forceinline__ size_t dcn_corner(const DcnSample& s, int q, size_t n, int H, int W, unsigned C) {
    return ((n * H + (size_t)(s.h0 + (q >> 1))) * W + (size_t)(s.w0 + (q & 1))) * C;
}

__device__ __forceinline__ float dcn_sigmoid(float l) { return 1.0f / (1.0f + expf(-l)); }

template <typename T>
__global__ __launch_bounds__(256) void dcn_cols_kernel(const T* __restrict__ x, const T* __restrict__ om,
                                                       T* __restrict__ cols, size_t chunks, int H, int W, unsigned C,
                                                       unsigned Cg, unsigned G, unsigned P, int sigmoid) {
    constexpr int E = Vec16<T>::N;
    const unsigned cpp = C / E;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (size_t)gridDim.x * 256) {
        const size_t t = i / cpp;                   // (pixel, tap)
        const unsigned ch = (unsigned)(i - t * cpp);
        const size_t pix = t / 9;
        const int k = (int)(t - pix * 9);
        const size_t row = pix / W;
        const int w = (int)(pix - row * W);
        const size_t n = row / H;
        const int h = (int)(row - n * H);
        const unsigned g = ch * E / Cg;             // Cg is a multiple of E: a chunk lies in one group
        const T* o = om + pix * P;
        const float dh = to_f<T>(o[18 * g + 2 * k]), dw = to_f<T>(o[18 * g + 2 * k + 1]);
        float m = to_f<T>(o[18 * G + 9 * g + k]);
        const DcnSample s = dcn_sample(h, w, k, dh, dw, H, W);
        float v[4][E];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (s.ok[q]) {
                Vec16<T>::load(x + dcn_corner(s, q, n, H, W, C) + (size_t)ch * E, v[q]);
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) v[q][e] = 0.0f;
            }
        }
        if (sigmoid) m = dcn_sigmoid(m);
        float r[E];
#pragma unroll
        for (int e = 0; e < E; ++e)
            r[e] = m * (((s.wt[0] * v[0][e] + s.wt[1] * v[1][e]) + s.wt[2] * v[2][e]) + s.wt[3] * v[3][e]);
        Vec16<T>::store(cols + i * E, r);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dcn_cols_bwd_kernel(const T* __restrict__ dcols, const T* __restrict__ x,
                                                           const T* __restrict__ om, float* __restrict__ dx,
                                                           T* __restrict__ dom, size_t items, int H, int W, unsigned C,
                                                           unsigned Cg, unsigned G, unsigned P, unsigned L,
                                                           int sigmoid) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned sub = lane / L, sl = lane - sub * L;     // L lanes per (pixel, tap, group); L a power of two
    const size_t per = 64 / L;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * 4;
    for (size_t base = wave * per; base < items; base += nwaves * per) {     // wave-uniform: the shuffles below
        const size_t it = base + sub;
        const bool live = it < items;
        float am = 0.0f, ah = 0.0f, aw = 0.0f, m = 0.0f;
        size_t pix = 0;
        unsigned g = 0;
        int k = 0;
        if (live) {
            const size_t t = it / G;
            g = (unsigned)(it - t * G);
            pix = t / 9;
            k = (int)(t - pix * 9);
            const size_t row = pix / W;
            const int w = (int)(pix - row * W);
            const size_t n = row / H;
            const int h = (int)(row - n * H);
            const T* o = om + pix * P;
            const float dh = to_f<T>(o[18 * g + 2 * k]), dw = to_f<T>(o[18 * g + 2 * k + 1]);
            m = to_f<T>(o[18 * G + 9 * g + k]);
            if (sigmoid) m = dcn_sigmoid(m);
            const DcnSample s = dcn_sample(h, w, k, dh, dw, H, W);
            size_t co[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) co[q] = s.ok[q] ? dcn_corner(s, q, n, H, W, C) + (size_t)g * Cg : 0;
            const T* dc = dcols + (pix * 9 + (size_t)k) * C + (size_t)g * Cg;
            for (unsigned c = sl; c < Cg; c += L) {
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = s.ok[q] ? to_f<T>(x[co[q] + c]) : 0.0f;
                const float d = to_f<T>(dc[c]);
                const float val = ((s.wt[0] * v[0] + s.wt[1] * v[1]) + s.wt[2] * v[2]) + s.wt[3] * v[3];
                am += d * val;
                ah += d * ((v[2] - v[0]) * (1.0f - s.lw) + (v[3] - v[1]) * s.lw);
                aw += d * ((v[1] - v[0]) * (1.0f - s.lh) + (v[3] - v[2]) * s.lh);
                const float dm = d * m;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (s.ok[q] && s.wt[q] != 0.0f) atomic_add_f32(dx + co[q] + c, dm * s.wt[q]);
            }
        }
        for (unsigned o = L >> 1; o > 0; o >>= 1) {
            am += __shfl_xor(am, o, 64);
            ah += __shfl_xor(ah, o, 64);
            aw += __shfl_xor(aw, o, 64);
        }
        if (live) {
            T* o = dom + pix * P;
            if (sl == 0) {
                o[18 * g + 2 * k] = from_f<T>(m * ah);
                o[18 * g + 2 * k + 1] = from_f<T>(m * aw);
                o[18 * G + 9 * g + k] = from_f<T>(sigmoid ? am * (m * (1.0f - m)) : am);
            }
            if (k == 0 && g == 0)
                for (unsigned c = 27 * G + sl; c < P; c += L) o[c] = from_f<T>(0.0f);
        }
    }
}

// extents > 0, G groups of a whole number of 16-byte chunks, P >= 27G channels in whole chunks, and columns that fit
// the 64-bit offsets with room
template <typename T>
bool dcn_args_ok(int N, int H, int W, int C, int G, int P, int sigmoid) {
    constexpr int E = 16 / sizeof(T);
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || P <= 0 || C % G || (C / G) % E) return false;
    if (G > (1 << 20) || P < 27 * G || P % E || (sigmoid != 0 && sigmoid != 1)) return false;
    return (double)N * H * W * 9.0 * C * 4.0 < 9.0e18 && (double)N * H * W * P * 4.0 < 9.0e18;
}

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool dcn_overlap(const void* a, double na, const void* b, double nb) {
    const double pa = (double)(uintptr_t)a, pb = (double)(uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

SCD_KERNEL_NS_END
}  // namespace

extern "C" int scd_dcn_cols(int dtype, const void* x, const void* om, void* cols, int N, int H, int W, int C, int G,
                            int P, int sigmoid, void* stream) {
    SCD_F16_FWD(scd_dcn_cols, x, om, cols, N, H, W, C, G, P, sigmoid, stream);
    if (!x || !om || !cols || cols == x || cols == om) return SCD_ERR_ARG;
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (!dcn_args_ok<T>(N, H, W, C, G, P, sigmoid)) return SCD_ERR_ARG;
        const double px = (double)N * H * W * sizeof(T);            // bytes of one channel over all pixels
        if (dcn_overlap(cols, 9.0 * C * px, x, C * px) || dcn_overlap(cols, 9.0 * C * px, om, P * px))
            return SCD_ERR_ARG;
        const size_t chunks = (size_t)N * H * W * 9 * (C / (16 / sizeof(T)));
        static const int res = resident_grid((const void*)dcn_cols_kernel<T>, 256);
        const int grid = (int)std::min<size_t>((size_t)res, (chunks + 255) / 256);
        hipLaunchKernelGGL((dcn_cols_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)om, (T*)cols, chunks, H, W, (unsigned)C, (unsigned)(C / G), (unsigned)G,
                           (unsigned)P, sigmoid);
        SCD_RETURN_LAUNCH();
    });
}

extern "C" int scd_dcn_cols_bwd(int dtype, const void* dcols, const void* x, const void* om, float* dx32, void* dom,
                                int N, int H, int W, int C, int G, int P, int sigmoid, void* stream) {
    SCD_F16_FWD(scd_dcn_cols_bwd, dcols, x, om, dx32, dom, N, H, W, C, G, P, sigmoid, stream);
    if (!dcols || !x || !om || !dx32 || !dom) return SCD_ERR_ARG;
    if (dom == dcols || dom == x || dom == om || (void*)dx32 == dcols || (void*)dx32 == x || (void*)dx32 == om ||
        (void*)dx32 == dom)
        return SCD_ERR_ARG;
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (!dcn_args_ok<T>(N, H, W, C, G, P, sigmoid)) return SCD_ERR_ARG;
        const double px = (double)N * H * W * sizeof(T), px32 = (double)N * H * W * 4.0;
        const void* in[3] = {dcols, x, om};
        const double inb[3] = {9.0 * C * px, C * px, P * px};
        for (int i = 0; i < 3; ++i)
            if (dcn_overlap(dom, P * px, in[i], inb[i]) || dcn_overlap(dx32, C * px32, in[i], inb[i]))
                return SCD_ERR_ARG;
        if (dcn_overlap(dx32, C * px32, dom, P * px)) return SCD_ERR_ARG;
        const unsigned Cg = (unsigned)(C / G);
        unsigned L = 4;
        while (L < 64 && L < Cg) L <<= 1;
        const size_t items = (size_t)N * H * W * 9 * G;
        const size_t waves = (items + 64 / L - 1) / (64 / L);
        static const int res = resident_grid((const void*)dcn_cols_bwd_kernel<T>, 256);
        const int grid = (int)std::min<size_t>((size_t)res, (waves + 3) / 4);
        hipLaunchKernelGGL((dcn_cols_bwd_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)dcols,
                           (const T*)x, (const T*)om, dx32, (T*)dom, items, H, W, (unsigned)C, Cg, (unsigned)G,
                           (unsigned)P, L, sigmoid);
        SCD_RETURN_LAUNCH();
    });
}
