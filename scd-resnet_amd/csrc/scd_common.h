// Shared device helpers for libscdhip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

// fp16 compute mode (SCD_DT_F16).  The type-generic sources (the Makefile's F16SRCS: conv_gemm, bn, layers, stem, pad,
// upsample, deform) are compiled twice:
// once as written (16-bit storage type h16 = __bf16, v_mfma_f32_16x16x32_bf16) and once with SCD_F16_BUILD, where h16
// is _Float16, the MFMA is v_mfma_f32_16x16x32_f16 and every entry point on the list below gets the symbol name
// name__f16.  Those sources name the 16-bit type h16 (and h16x8 / mfma_16x16x32_h16) wherever it is the build's type;
// __bf16 in them is always a real bf16, whichever build.  A call with dtype SCD_DT_F16 is forwarded by the first build
// to the second with dtype SCD_DT_BF16 ("the 16-bit type") by SCD_F16_FWD, the first line of each listed entry point,
// so every kernel, tile shape and dispatch rule is shared and the C-ABI takes SCD_DT_F16 like any other dtype.
// The second build holds the listed entry points and what they launch, nothing else: an entry point without a dtype
// (and the kernels only it launches) sits in its file's one `#ifndef SCD_F16_BUILD` region, and the fp32 kernels are
// named only through scd_dispatch_dtype's float arm, which that build does not have.
#include "../../include/scdhip.h"

// the entry points that take a dtype: this list is the only one (tests/test_host_cpu.py holds the SCD_F16_FWD lines
// to it)
#define SCD_F16_ENTRY_POINTS(X) \
    X(scd_conv_gemm) \
    X(scd_conv_gemm_sel) \
    X(scd_conv_gemm_bnbwd) \
    X(scd_conv_gemm_res) \
    X(scd_conv_gemm_heads) \
    X(scd_conv_gemm_heads_keep) \
    X(scd_conv_wgrad_nsplit2) \
    X(scd_conv_wgrad_nsplit) \
    X(scd_conv_wgrad) \
    X(scd_bn_apply) \
    X(scd_bn_bwd_reduce) \
    X(scd_bn_bwd_apply) \
    X(scd_bn_bwd_reduce2) \
    X(scd_bn_bwd_apply2) \
    X(scd_pack_weights_batched) \
    X(scd_pack_weight) \
    X(scd_im2col_stem) \
    X(scd_stem_pool_fwd) \
    X(scd_stem_pool_bwd) \
    X(scd_stem_pool_bwd_bn) \
    X(scd_heads_fwd) \
    X(scd_heads_bwd) \
    X(scd_heads_bwd_packed) \
    X(scd_heads_bwd_packed_split) \
    X(scd_heads_sparse_bwd) \
    X(scd_heads_sparse_fixup) \
    X(scd_stem_conv_fwd) \
    X(scd_stem_conv_wgrad) \
    X(scd_stem_bwd_fused) \
    X(scd_conv_dgrad_s2) \
    X(scd_stem_bwd_combine) \
    X(scd_pad_channels) \
    X(scd_upsample2x_add) \
    X(scd_upsample2x_add_bwd) \
    X(scd_dcn_cols) \
    X(scd_dcn_cols_bwd)
#ifdef SCD_F16_BUILD
// (the preprocessor cannot write a #define per list item: the second build's definitions, and its calls from one
// listed entry point to another, get their symbol name from this redeclaration)
#define SCD_F16_RENAME(fn) extern "C" decltype(fn) fn __asm__(#fn "__f16");
SCD_F16_ENTRY_POINTS(SCD_F16_RENAME)
#define SCD_F16_FWD(fn, ...) ((void)0)
#else
#define SCD_F16_DECL(fn) extern "C" decltype(fn) fn##__f16;
SCD_F16_ENTRY_POINTS(SCD_F16_DECL)
#define SCD_F16_FWD(fn, ...) \
    do { if (dtype == SCD_DT_F16) return fn##__f16(SCD_DT_BF16, __VA_ARGS__); } while (0)
#endif

// The fp16 build's kernels sit in an inline namespace `f16` inside each file's anonymous namespace, so their symbol
// names (and the rocprofv3 kernel names) differ from the bf16 build's even where a kernel is not templated on the
// 16-bit type (tools/prof_summary.py labels them by it).
#ifdef SCD_F16_BUILD
#define SCD_KERNEL_NS_BEGIN inline namespace f16 {
#define SCD_KERNEL_NS_END }
#else
#define SCD_KERNEL_NS_BEGIN
#define SCD_KERNEL_NS_END
#endif

// half `hi` of a 32-bit word holding two 16-bit values, as float
__device__ __forceinline__ float h16_word_half(unsigned w, int hi) {
#ifdef SCD_F16_BUILD
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(hi ? w >> 16 : w & 0xffffu));
#else
    return __uint_as_float(hi ? (w & 0xffff0000u) : (w << 16));
#endif
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;     // a real bf16 vector in either build
#ifdef SCD_F16_BUILD
typedef _Float16 h16;                                           // the build's 16-bit compute type
#else
typedef __bf16 h16;
#endif
typedef __attribute__((ext_vector_type(8))) h16 h16x8;
typedef __attribute__((ext_vector_type(4))) h16 h16x4;
// v_mfma_f32_16x16x32_{bf16,f16} on the build's 16-bit type
__device__ __forceinline__ f32x4 mfma_16x16x32_h16(h16x8 a, h16x8 b, f32x4 c) {
#ifdef SCD_F16_BUILD
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#endif
}
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// The one dtype dispatch of the typed entry points: f(scd_type<T>{}) with T = h16 for SCD_DT_BF16 (the build's 16-bit
// type) or float for SCD_DT_F32, SCD_ERR_ARG for any other dtype.  The fp16 build only ever receives the 16-bit type
// and has no float arm, so it instantiates no fp32 kernel.
template <typename T> struct scd_type { using type = T; };
template <typename F>
static inline int scd_dispatch_dtype(int dtype, F&& f) {
    if (dtype == SCD_DT_BF16) return f(scd_type<h16>{});
#ifndef SCD_F16_BUILD
    if (dtype == SCD_DT_F32) return f(scd_type<float>{});
#endif
    return SCD_ERR_ARG;
}

#define SCD_RETURN_LAUNCH() return (int)hipGetLastError()

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<h16>(h16 v) { return (float)v; }

template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ h16 from_f<h16>(float v) { return (h16)v; }

// 16-byte vector of T <-> floats
template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int N = 4;
    __device__ static void load(const void* p, float* f) {
        float4 v = *(const float4*)p;
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
    __device__ static void store(void* p, const float* f) {
        *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
    }
};
template <> struct Vec16<h16> {
    static constexpr int N = 8;
    __device__ static void load(const void* p, float* f) {
        h16x8 v = *(const h16x8*)p;
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
    }
    __device__ static void store(void* p, const float* f) {
        h16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (h16)f[i];
        *(h16x8*)p = v;
    }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fp64 atomic add (global_atomic_add_f64 on gfx950)
__device__ __forceinline__ void atomic_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Compute units of the current device (256 when the query fails), asked once per process
static inline int num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
    }
    return n;
}

// Workgroups of `kernel` (blockDim `threads`, no dynamic LDS) resident on the whole device at once:
// grid-stride HBM kernels launch exactly this many, so every workgroup runs in the first (only) round
// and the grid never has a partial second round.
static inline int resident_grid(const void* kernel, int threads, size_t dyn_lds = 0) {
    int per = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, dyn_lds) != hipSuccess || per < 1) per = 1;
    return per * num_cus();
}
