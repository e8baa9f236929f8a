// The hourglass up path (models/backbones/hourglass.py:113-114 of the reference): Upsample(scale_factor=2, nearest)
// fused with MergeUp, and its backward, on NHWC activations.
//   forward   out[n][2i+a][2j+b][c] = up[n][2i+a][2j+b][c] + low[n][i][j][c]        (fp32 sum, one rounding)
//   backward  dlow[n][i][j][c] = (d00 + d01) + (d10 + d11) of dout's 2x2 block      (fp32, this order, one rounding)
// The gradient towards `up` is dout itself: no kernel.  Both are HBM-bound streams (forward 9, backward 5 units of
// N*h*w*C elements): one thread owns one 16-byte channel chunk of one low pixel, issues its five (four) vector loads
// before it uses any of them, and a grid of resident workgroups strides over the chunks.  No atomics, no LDS.
#include <algorithm>

#include "scd_common.h"

namespace {
SCD_KERNEL_NS_BEGIN

// element offset of chunk `ch` of the top-left pixel of low pixel `pix`'s 2x2 block in the (N, 2h, 2w, C) tensor;
// pix = (n*h + i)*w + j, so the block's first row is 2*(n*h + i) of the N*2h rows of 2w pixels
template <int E>
__device__ __forceinline__ size_t block_origin(size_t pix, unsigned ch, unsigned w, unsigned C) {
    const size_t row = pix / w;
    const size_t j = pix - row * w;
    return ((row * 2) * (2 * (size_t)w) + 2 * j) * C + (size_t)ch * E;
}

template <typename T>
__global__ __launch_bounds__(256) void upsample2x_add_kernel(const T* __restrict__ up, const T* __restrict__ low,
                                                             T* __restrict__ out, size_t chunks, unsigned w,
                                                             unsigned C) {
    constexpr int E = Vec16<T>::N;
    const unsigned cpp = C / E;
    const size_t rs = 2 * (size_t)w * C;                // one row of the upsampled tensor
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / cpp;
        const unsigned ch = (unsigned)(i - pix * cpp);
        const size_t o = block_origin<E>(pix, ch, w, C);
        float l[E], u[4][E];
        Vec16<T>::load(low + i * E, l);
        Vec16<T>::load(up + o, u[0]);
        Vec16<T>::load(up + o + C, u[1]);
        Vec16<T>::load(up + o + rs, u[2]);
        Vec16<T>::load(up + o + rs + C, u[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < E; ++e) u[k][e] += l[e];
        }
        Vec16<T>::store(out + o, u[0]);
        Vec16<T>::store(out + o + C, u[1]);
        Vec16<T>::store(out + o + rs, u[2]);
        Vec16<T>::store(out + o + rs + C, u[3]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void upsample2x_add_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dlow,
                                                                 size_t chunks, unsigned w, unsigned C) {
    constexpr int E = Vec16<T>::N;
    const unsigned cpp = C / E;
    const size_t rs = 2 * (size_t)w * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / cpp;
        const unsigned ch = (unsigned)(i - pix * cpp);
        const size_t o = block_origin<E>(pix, ch, w, C);
        float d[4][E];
        Vec16<T>::load(dout + o, d[0]);
        Vec16<T>::load(dout + o + C, d[1]);
        Vec16<T>::load(dout + o + rs, d[2]);
        Vec16<T>::load(dout + o + rs + C, d[3]);
#pragma unroll
        for (int e = 0; e < E; ++e) d[0][e] = (d[0][e] + d[1][e]) + (d[2][e] + d[3][e]);
        Vec16<T>::store(dlow + i * E, d[0]);
    }
}

// extents > 0, C a multiple of the 16-byte chunk, and N*h*w*(C/E) chunks that fit the 64-bit offsets with room
template <typename T>
bool upsample_args_ok(int N, int h, int w, int C, size_t& chunks) {
    constexpr int E = 16 / sizeof(T);
    if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || C % E) return false;
    if ((double)N * h * w * C * 4.0 >= 9.0e18) return false;
    chunks = (size_t)N * h * w * (C / E);
    return true;
}
inline int stream_grid(int resident, size_t chunks) {
    return (int)std::min<size_t>((size_t)resident, (chunks + 255) / 256);
}

SCD_KERNEL_NS_END
}  // namespace

extern "C" int scd_upsample2x_add(int dtype, const void* up, const void* low, void* out, int N, int h, int w, int C,
                                  void* stream) {
    SCD_F16_FWD(scd_upsample2x_add, up, low, out, N, h, w, C, stream);
    // `up` is a residual block's output, kept by that block as its ReLU mask: the merge never writes over an operand
    if (!up || !low || !out || out == up || out == low) return SCD_ERR_ARG;
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        size_t chunks;
        if (!upsample_args_ok<T>(N, h, w, C, chunks)) return SCD_ERR_ARG;
        static const int g = resident_grid((const void*)upsample2x_add_kernel<T>, 256);
        hipLaunchKernelGGL((upsample2x_add_kernel<T>), dim3(stream_grid(g, chunks)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)up, (const T*)low, (T*)out, chunks, (unsigned)w, (unsigned)C);
        SCD_RETURN_LAUNCH();
    });
}

extern "C" int scd_upsample2x_add_bwd(int dtype, const void* dout, void* dlow, int N, int h, int w, int C,
                                      void* stream) {
    SCD_F16_FWD(scd_upsample2x_add_bwd, dout, dlow, N, h, w, C, stream);
    if (!dout || !dlow || dout == dlow) return SCD_ERR_ARG;
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        size_t chunks;
        if (!upsample_args_ok<T>(N, h, w, C, chunks)) return SCD_ERR_ARG;
        static const int g = resident_grid((const void*)upsample2x_add_bwd_kernel<T>, 256);
        hipLaunchKernelGGL((upsample2x_add_bwd_kernel<T>), dim3(stream_grid(g, chunks)), dim3(256), 0,
                           (hipStream_t)stream, (const T*)dout, (T*)dlow, chunks, (unsigned)w, (unsigned)C);
        SCD_RETURN_LAUNCH();
    });
}
