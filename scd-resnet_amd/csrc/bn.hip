// Training-mode BatchNorm2d pieces for NHWC activations (residuals.py:92,95,212,262,306).
// Statistics are accumulated in fp64 into SCD_STAT_REPLICAS replicas (spreads the atomics),
// finalised per channel; apply / backward passes are 16-byte-vectorised elementwise kernels.
#include <algorithm>
#include <type_traits>

#include "scd_common.h"

#ifndef BN_BWD_U
#define BN_BWD_U 1
#endif
// Elementwise BN kernels are budgeted for 6 waves per SIMD (<= 80 VGPRs): the weight-gradient stream's ping-pong
// kernel holds 2 x 216 of the 512 VGPRs per SIMD lane (one 8-wave workgroup per CU), so a wave that needs 88 could
// not start on any CU until those workgroups retire (in the step the deconv2 BN backward apply then waited out the
// whole deconv3 weight gradient)
// vectors in flight per thread in the one-layer bn_bwd_apply_kernel (80 VGPRs at 2, no spill): beside the
// weight-gradient stream's one-workgroup-per-CU GEMM a CU holds one or two of its waves per SIMD, so the bytes each
// wave keeps in flight set its bandwidth there (75 VGPRs at 2 in both 16-bit builds since the loop is specialised per
// mask kind)
#ifndef BN_APPLY_U
#define BN_APPLY_U 2
#endif
#ifndef BN_EW_WAVES
#define BN_EW_WAVES 6
#endif

namespace {
SCD_KERNEL_NS_BEGIN

// E consecutive per-channel floats (E = 4 or 8, 16-B aligned) as float4 loads
template <int E>
__device__ __forceinline__ void load_params(const float* p, float* v) {
#pragma unroll
    for (int k = 0; k < E / 4; ++k) {
        const float4 f = *(const float4*)(p + 4 * k);
        v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
    }
}

// Per-channel parameters of the backward kernels live in LDS and are re-read per vector instead of held in
// registers (5-6 x E floats per thread otherwise): with <= 80 VGPRs (BN_EW_WAVES) the waves fit beside the
// weight-gradient stream's one-workgroup-per-CU GEMMs.  The offset is made opaque so the reads stay in the loop.
// Only the channels a block touches are staged (chan_window): at most 256 chunks of E channels, so the dynamic LDS is
// bounded (<= 6 x 2048 x 4 B for bf16) whatever C is, and the host sizes the grid with that LDS in the occupancy query.
__device__ __forceinline__ void stage_params(float* sp, const float* const* src, int nsrc, int cb, int W) {
    for (int i = threadIdx.x; i < nsrc * W; i += blockDim.x) {
        const int k = i / W;
        sp[i] = src[k] ? src[k][cb + i - k * W] : 0.f;
    }
    __syncthreads();
}
// first channel and width of the channel window of this block's threads in the elementwise kernels (one fixed chunk
// of E channels per thread, grid stride a multiple of the C/E chunks per row, ew_rows_ok): the whole row when it has
// <= 256 chunks, else the block's own 256-chunk window
__device__ __forceinline__ void chan_window(int C, int E, int& cb, int& W) {
    const unsigned cpr = (unsigned)C / E;
    cb = cpr > 256u ? (int)((blockIdx.x * 256u) % cpr) * E : 0;
    W = cpr > 256u ? 256 * E : C;
}
template <int E>
__device__ __forceinline__ void lds_params(const float* sp, int off, float* v) {
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int k = 0; k < E / 4; ++k) {
        const float4 f = *(const float4*)(sp + off + 4 * k);
        v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* y, T* out, int C, unsigned nvec, const float* scale,
                                                       const float* shift, const T* res, const float* rscale,
                                                       const float* rshift, int relu) {
    constexpr int E = Vec16<T>::N;
    constexpr int U = 4;
    // the grid stride is a multiple of the chunks per row (ew_rows_ok, ew_grid): a thread always owns the same
    // E channels, so the per-channel parameters live in registers (no LDS, no bank conflicts).  U vectors
    // per thread are loaded before any is used (U x 16 B, x2 with a residual, in flight per thread).
    const unsigned cpr = (unsigned)C / E;
    const unsigned v0 = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned stride = gridDim.x * blockDim.x;
    const int c0 = (int)(v0 % cpr) * E;
    float sc[E], sh[E], rs[E], rh[E];
    load_params<E>(scale + c0, sc);
    load_params<E>(shift + c0, sh);
    if (rscale) { load_params<E>(rscale + c0, rs); load_params<E>(rshift + c0, rh); }
    else {
#pragma unroll
        for (int e = 0; e < E; ++e) { rs[e] = 0.f; rh[e] = 0.f; }
    }
    auto body = [&](float* a, const float* r) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            float o = a[e] * sc[e] + sh[e];
            if (res) o += rscale ? (r[e] * rs[e] + rh[e]) : r[e];
            if (relu) o = fmaxf(o, 0.f);
            a[e] = o;
        }
    };
    unsigned v = v0;
    for (; v + (U - 1) * stride < nvec; v += U * stride) {
        float a[U][E], r[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            Vec16<T>::load(y + (size_t)(v + u * stride) * E, a[u]);
            if (res) Vec16<T>::load(res + (size_t)(v + u * stride) * E, r[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            body(a[u], r[u]);
            Vec16<T>::store(out + (size_t)(v + u * stride) * E, a[u]);
        }
    }
    for (; v < nvec; v += stride) {
        float a[E], r[E];
        Vec16<T>::load(y + (size_t)v * E, a);
        if (res) Vec16<T>::load(res + (size_t)v * E, r);
        body(a, r);
        Vec16<T>::store(out + (size_t)v * E, a);
    }
}

// ---- BatchNorm backward, for one layer (NL = 1) or for the two layers behind one residual join (NL = 2: BasicBlock /
// Bottleneck bn2|bn3 + downsample BN, residuals.py:110-120, 158-165; CornerPool branchMergeBn + shortcutBn,
// cornerNetCPool.py:117-122).  Both layers of a pair take the same gradient dout through the same stored ReLU mask, so
// one pass reads dout and the mask once for both.  The layer count is a template parameter of the same kernels: per
// element and per thread a pair pass computes what two single passes with that mask compute.
//
// Kernel arguments.  NL = 1 has the three mask kinds (0: none, 1: the stored activation `mask`, 2: BN+ReLU recomputed
// from y with rsc / rsh); NL = 2 has kind 1 only (the host rejects a null mask).
template <typename T, int NL> struct BwdReduceArgs;
template <typename T> struct BwdReduceArgs<T, 1> {
    const T *dout, *mask, *y[1];
    const float *rsc, *rsh, *mi[2];                 // mi: mean, invstd
    int C, ld;
    unsigned rows, rows_per_block;
    double* stats[1];
};
template <typename T> struct BwdReduceArgs<T, 2> {
    const T *dout, *mask, *y[2];
    const float* mi[4];                             // mean_a, invstd_a, mean_b, invstd_b
    int C, ld;
    unsigned rows, rows_per_block;
    double* stats[2];
};
template <typename T, int NL> struct BwdApplyArgs;
template <typename T> struct BwdApplyArgs<T, 1> {
    const T *dout, *mask, *y[1];
    const float *rsc, *rsh, *coef[1];
    int C;
    unsigned nvec;
    T *dy[1], *dz;                                  // dz: optional, the masked gradient
};
template <typename T> struct BwdApplyArgs<T, 2> {
    const T *dout, *mask, *y[2];
    const float* coef[2];
    int C;
    unsigned nvec;
    T* dy[2];
};
// per-channel arrays bn_bwd_apply_kernel stages: 3 coefficients per layer, and rsc, rsh of the one layer
constexpr int bwd_apply_nsrc(int NL) { return NL == 1 ? 5 : 6; }

// one step's operands as loaded, packed (16 B each) until used: dout, the stored activation (mask kind 1), NL layers' y
template <int NL> struct BwdRaw { uint4 d, m, y[NL]; };
template <int MK, typename T, int NL>
__device__ __forceinline__ void load_bwd_raw(const T* dout, const T* mask, const T* const (&y)[NL], size_t i,
                                             BwdRaw<NL>& raw) {
    raw.d = *(const uint4*)(dout + i);
#pragma unroll
    for (int l = 0; l < NL; ++l) raw.y[l] = *(const uint4*)(y[l] + i);
    raw.m = MK == 1 ? *(const uint4*)(mask + i) : make_uint4(0, 0, 0, 0);
}

// The loop of the backward kernels over steps i, i + stride, .. < end: U steps are loaded before any is used (U x the
// step's 16-B loads in flight per thread), then a ragged tail one step at a time.
template <int U, typename Raw, typename Load, typename Use>
__device__ __forceinline__ void loads_ahead_loop(unsigned i, unsigned end, unsigned stride, Load load, Use use) {
    for (; i + (U - 1) * stride < end; i += U * stride) {
        Raw raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) load(i + u * stride, raw[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) use(i + u * stride, raw[u]);
    }
    if constexpr (U > 1) {
        for (; i < end; i += stride) {
            Raw raw;
            load(i, raw);
            use(i, raw);
        }
    }
}
// one loop per mask kind: with the kind a runtime test inside the element loop the compiler built the loop from
// per-element branch regions (8 per vector)
template <int NL, typename Args, typename Run>
__device__ __forceinline__ void per_mask_kind(const Args& a, Run run) {
    if constexpr (NL == 2) {
        run(std::integral_constant<int, 1>{});
    } else {
        if (a.mask) run(std::integral_constant<int, 1>{});
        else if (a.rsc) run(std::integral_constant<int, 2>{});
        else run(std::integral_constant<int, 0>{});
    }
}

// Per-channel Σdz and, per layer, Σdz·x̂ over rows (dz = dout masked by relu(mask) > 0).  A 256-thread block owns
// rows [r0, r1): thread = (row lane rsub, 16-B channel chunk ch); BN_BWD_U rows per step are loaded before any is
// used; the block's partials are folded over row lanes in LDS by all threads and added to one fp64 replica slot per
// channel (Σdz to every layer's).
template <typename T, int NL>
__global__ __launch_bounds__(256, BN_EW_WAVES) void bn_bwd_reduce_kernel(BwdReduceArgs<T, NL> a) {
    constexpr int E = Vec16<T>::N;
    constexpr int nt = 256;
    const int C = a.C, ld = a.ld;
    const int cpr = C / E;                     // chunks per row of this channel slice (<= 256)
    const int rpi = nt / cpr;                  // row lanes
    const int tid = threadIdx.x;
    const int ch = tid % cpr;
    const int rsub = tid / cpr;
    const bool lane = rsub < rpi;              // false for the block's last 256 % cpr threads: no row lane, no rows
    const unsigned r0 = blockIdx.x * a.rows_per_block;
    const unsigned r1 = min(a.rows, r0 + a.rows_per_block);
    __shared__ float red[2 * nt * E];
    // 4 x C floats (dynamic LDS): mean, invstd, rsc, rsh | mean_a, invstd_a, mean_b, invstd_b
    extern __shared__ __attribute__((aligned(16))) float sp[];
    {
        const float* src[4] = {a.mi[0], a.mi[1]};
        if constexpr (NL == 1) { src[2] = a.rsc; src[3] = a.rsh; }
        else { src[2] = a.mi[2]; src[3] = a.mi[3]; }
        stage_params(sp, src, 4, 0, C);
    }
    float s[E], q[NL][E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        s[e] = 0.f;
#pragma unroll
        for (int l = 0; l < NL; ++l) q[l][e] = 0.f;
    }
    per_mask_kind<NL>(a, [&](auto kind) {
        constexpr int MK = decltype(kind)::value;
        auto load = [&](unsigned r, BwdRaw<NL>& raw) {
            load_bwd_raw<MK>(a.dout, a.mask, a.y, r * (unsigned)ld + ch * E, raw);
        };
        auto acc = [&](unsigned, const BwdRaw<NL>& raw) {
            float d[E], yv[NL][E], mk[E], mu[E], is[E], ka[E], kb[E];
            Vec16<T>::load(&raw.d, d);
#pragma unroll
            for (int l = 0; l < NL; ++l) Vec16<T>::load(&raw.y[l], yv[l]);
            if constexpr (MK == 1) Vec16<T>::load(&raw.m, mk);
            lds_params<E>(sp, ch * E, mu);
            lds_params<E>(sp, C + ch * E, is);
            if constexpr (MK == 2) { lds_params<E>(sp, 2 * C + ch * E, ka); lds_params<E>(sp, 3 * C + ch * E, kb); }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                bool off = false;
                if constexpr (MK == 1) off = !(mk[e] > 0.f);
                if constexpr (MK == 2) off = !(yv[0][e] * ka[e] + kb[e] > 0.f);
                d[e] = off ? 0.f : d[e];
                s[e] += d[e];
                q[0][e] += d[e] * (yv[0][e] - mu[e]) * is[e];
            }
            if constexpr (NL == 2) {
                lds_params<E>(sp, 2 * C + ch * E, mu);
                lds_params<E>(sp, 3 * C + ch * E, is);
#pragma unroll
                for (int e = 0; e < E; ++e) q[1][e] += d[e] * (yv[1][e] - mu[e]) * is[e];
            }
        };
        loads_ahead_loop<BN_BWD_U, BwdRaw<NL>>(lane ? r0 + rsub : r1, r1, rpi, load, acc);
    });
    const int rep = (int)(blockIdx.x % SCD_STAT_REPLICAS);   // (mirrors stat_replica / stat_slot, gemm_common.h)
    // red[stat][rsub][channel].  Pass 1: sum dz (every layer's) and layer 0's sum dz*xhat; pass 2: layer 1's
    if (lane) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            red[rsub * C + ch * E + e] = s[e];
            red[nt * E + rsub * C + ch * E + e] = q[0][e];
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += nt) {
        double ss = 0.0, qq = 0.0;
        for (int k = 0; k < rpi; ++k) {
            ss += red[k * C + c];
            qq += red[nt * E + k * C + c];
        }
        atomic_add_f64(a.stats[0] + ((long)rep * 2 + 0) * ld + c, ss);
        atomic_add_f64(a.stats[0] + ((long)rep * 2 + 1) * ld + c, qq);
        if constexpr (NL == 2) atomic_add_f64(a.stats[1] + ((long)rep * 2 + 0) * ld + c, ss);
    }
    if constexpr (NL == 2) {
        __syncthreads();
        if (lane) {
#pragma unroll
            for (int e = 0; e < E; ++e) red[nt * E + rsub * C + ch * E + e] = q[1][e];
        }
        __syncthreads();
        for (int c = tid; c < C; c += nt) {
            double qq = 0.0;
            for (int k = 0; k < rpi; ++k) qq += red[nt * E + k * C + c];
            atomic_add_f64(a.stats[1] + ((long)rep * 2 + 1) * ld + c, qq);
        }
    }
}

// dy = a*dz + b*y + c per layer (and dz itself, NL = 1 with a.dz).  Vectors in flight, kept packed until used:
// BN_APPLY_U for one layer, BN_BWD_U for a pair (twice the operands per step): <= 80 VGPRs, so the kernel's waves fit
// beside a one-workgroup-per-CU GEMM of the weight-gradient stream (2 x 216 of the 512 VGPRs per lane) instead of
// waiting for its workgroups to retire
template <typename T, int NL>
__global__ __launch_bounds__(256, BN_EW_WAVES) void bn_bwd_apply_kernel(BwdApplyArgs<T, NL> a) {
    constexpr int E = Vec16<T>::N;
    constexpr int U = NL == 1 ? BN_APPLY_U : BN_BWD_U;
    constexpr int NS = bwd_apply_nsrc(NL);
    // fixed channel chunk per thread (see bn_apply_kernel)
    const int C = a.C;
    const unsigned cpr = (unsigned)C / E;
    const unsigned v0 = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned stride = gridDim.x * blockDim.x;
    const int c0 = (int)(v0 % cpr) * E;
    // NS x W floats (dynamic LDS): coef a, b, c, rsc, rsh | coef_a a, b, c, coef_b a, b, c
    extern __shared__ __attribute__((aligned(16))) float sp[];
    int cb, W;
    chan_window(C, E, cb, W);
    if constexpr (NL == 1) {
        const float* src[NS] = {a.coef[0], a.coef[0] + C, a.coef[0] + 2 * C, a.rsc, a.rsh};
        stage_params(sp, src, NS, cb, W);
    } else {
        const float* src[NS] = {a.coef[0], a.coef[0] + C, a.coef[0] + 2 * C,
                                a.coef[1], a.coef[1] + C, a.coef[1] + 2 * C};
        stage_params(sp, src, NS, cb, W);
    }
    const int cl = c0 - cb;
    per_mask_kind<NL>(a, [&](auto kind) {
        constexpr int MK = decltype(kind)::value;
        auto load = [&](unsigned v, BwdRaw<NL>& raw) { load_bwd_raw<MK>(a.dout, a.mask, a.y, (size_t)v * E, raw); };
        // raw 16-B vectors -> dz (masked gradient) and dy, stored
        auto body = [&](unsigned v, const BwdRaw<NL>& raw) {
            const size_t i = (size_t)v * E;
            float d[E], yv[NL][E], mk[E], k0[E], k1[E], k2[E], ka[E], kb[E];
            Vec16<T>::load(&raw.d, d);
#pragma unroll
            for (int l = 0; l < NL; ++l) Vec16<T>::load(&raw.y[l], yv[l]);
            if constexpr (MK == 1) Vec16<T>::load(&raw.m, mk);
            lds_params<E>(sp, cl, k0);
            lds_params<E>(sp, W + cl, k1);
            lds_params<E>(sp, 2 * W + cl, k2);
            if constexpr (MK == 2) { lds_params<E>(sp, 3 * W + cl, ka); lds_params<E>(sp, 4 * W + cl, kb); }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                bool off = false;
                if constexpr (MK == 1) off = !(mk[e] > 0.f);
                if constexpr (MK == 2) off = !(yv[0][e] * ka[e] + kb[e] > 0.f);
                d[e] = off ? 0.f : d[e];
                yv[0][e] = k0[e] * d[e] + k1[e] * yv[0][e] + k2[e];
            }
            if constexpr (NL == 2) {
                lds_params<E>(sp, 3 * W + cl, k0);
                lds_params<E>(sp, 4 * W + cl, k1);
                lds_params<E>(sp, 5 * W + cl, k2);
#pragma unroll
                for (int e = 0; e < E; ++e) yv[1][e] = k0[e] * d[e] + k1[e] * yv[1][e] + k2[e];
            }
#pragma unroll
            for (int l = 0; l < NL; ++l) Vec16<T>::store(a.dy[l] + i, yv[l]);
            if constexpr (NL == 1) {
                if (a.dz) Vec16<T>::store(a.dz + i, d);
            }
        };
        loads_ahead_loop<U, BwdRaw<NL>>(v0, a.nvec, stride, load, body);
    });
}

// elementwise BN kernels keep one channel chunk per thread: the grid stride (grid * 256 threads) must be a
// multiple of the chunks per row cpr.  Three kinds of row: cpr divides 256 (any grid), cpr is a multiple of 256 (grid a
// multiple of cpr / 256), and rows of whole 128-byte lines below 256 chunks (cpr a multiple of 8: the hourglass's 192
// channels are 24 bf16 / 48 fp32 chunks), whose grid is a multiple of cpr / gcd(cpr, 256) and whose reduction leaves
// the last 256 % cpr threads of a block without a row lane.  Other widths (3 chunks, 12, ..) stay refused.
inline bool ew_rows_ok(int cpr) {
    return cpr > 0 && (256 % cpr == 0 || cpr % 256 == 0 || (cpr < 256 && cpr % 8 == 0));
}
inline long ew_grid_unit(int cpr) {
    if (cpr > 256) return cpr / 256;
    return cpr / (cpr & -cpr);                      // cpr <= 256: gcd(cpr, 256) is the largest power of two in cpr
}
inline int ew_grid(int resident, long nvec, int cpr) {
    const long m = ew_grid_unit(cpr);
    long g = std::min<long>(resident, (nvec + 255) / 256);
    g = std::max<long>(m, g / m * m);
    return (int)g;
}
// dynamic LDS of an elementwise backward kernel staging nsrc per-channel arrays over its channel window (chan_window)
inline size_t ew_param_lds(int nsrc, int C, int E) { return (size_t)nsrc * std::min(C, 256 * E) * sizeof(float); }
constexpr size_t EW_LDS_MAX = 64 * 1024;
// resident blocks of Kernel with `lds` bytes of dynamic LDS, cached per kernel and window width
template <auto Kernel>
inline int ew_resident(size_t lds) {
    static int cache[EW_LDS_MAX / 16 + 1] = {0};        // lds is a multiple of 16 B (E >= 4 floats per chunk)
    const size_t k = std::min<size_t>(lds / 16, EW_LDS_MAX / 16);
    if (!cache[k]) cache[k] = resident_grid((const void*)Kernel, 256, lds);
    return cache[k];
}

// The backward reduce of a.C channels over total / a.C rows (a.ld, rows and rows_per_block are filled in here).  Rows
// wider than 256 chunks run as channel slices of 256 chunks (ld = the full row).  One round of resident blocks (at
// most), at least 8 rows per row lane; the grid is sized from the residency of the NL = 1 kernel for either layer
// count, so a pair pass partitions the rows, and with them every thread's partial sums, like two single passes.
template <typename T, int NL>
int launch_bwd_reduce(BwdReduceArgs<T, NL> a, long total, void* stream) {
    constexpr int E = 16 / sizeof(T);
    const int C = a.C;
    if (C % E || !ew_rows_ok(C / E) || total >= (1L << 31)) return SCD_ERR_ARG;
    const long rows = total / C;
    const int scpr = std::min(C / E, 256), sC = scpr * E;
    const size_t lds = (size_t)4 * sC * sizeof(float);
    const long nb = ew_resident<bn_bwd_reduce_kernel<T, 1>>(lds);
    const long rpi = 256 / scpr;
    const long rpb = std::max<long>(8 * rpi, (rows + nb - 1) / nb + rpi - 1) / rpi * rpi;
    const int blocks = cdiv(rows, rpb);
    a.C = sC;
    a.ld = C;
    a.rows = (unsigned)rows;
    a.rows_per_block = (unsigned)rpb;
    auto next_slice = [sC](auto*& p) { if (p) p += sC; };
    for (int c0 = 0; c0 < C; c0 += sC) {
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, NL>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        next_slice(a.dout);
        next_slice(a.mask);
        if constexpr (NL == 1) { next_slice(a.rsc); next_slice(a.rsh); }
        for (auto& p : a.y) next_slice(p);
        for (auto& p : a.mi) next_slice(p);
        for (auto& p : a.stats) next_slice(p);
    }
    return 0;
}

// the backward apply of total elements in rows of a.C channels (a.nvec is filled in here)
template <typename T, int NL>
int launch_bwd_apply(BwdApplyArgs<T, NL> a, long total, void* stream) {
    constexpr int E = 16 / sizeof(T);
    if (a.C % E || !ew_rows_ok(a.C / E)) return SCD_ERR_ARG;
    const long nvec = total / E;
    const size_t lds = ew_param_lds(bwd_apply_nsrc(NL), a.C, E);
    if (lds > EW_LDS_MAX) return SCD_ERR_ARG;
    a.nvec = (unsigned)nvec;
    const int g = ew_resident<bn_bwd_apply_kernel<T, NL>>(lds);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, NL>), dim3(ew_grid(g, nvec, a.C / E)), dim3(256), lds,
                       (hipStream_t)stream, a);
    SCD_RETURN_LAUNCH();
}

SCD_KERNEL_NS_END
}  // namespace

extern "C" int scd_bn_apply(int dtype, const void* y, void* out, int C, long total, const float* scale,
                            const float* shift, const void* res, const float* rscale, const float* rshift, int relu,
                            void* stream) {
    SCD_F16_FWD(scd_bn_apply, y, out, C, total, scale, shift, res, rscale, rshift, relu, stream);
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        constexpr int E = 16 / sizeof(T);
        if (C % E || !ew_rows_ok(C / E)) return SCD_ERR_ARG;
        long nvec = total / E;
        static const int g = resident_grid((const void*)bn_apply_kernel<T>, 256);
        hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(ew_grid(g, nvec, C / E)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)y, (T*)out, C, (unsigned)nvec, scale, shift, (const T*)res, rscale, rshift, relu);
        SCD_RETURN_LAUNCH();
    });
}

extern "C" int scd_bn_bwd_reduce(int dtype, const void* dout, const void* mask, const void* y, const float* relu_scale,
                                 const float* relu_shift, const float* mean,
                                 const float* invstd, int C, long total, double* stats, void* stream) {
    SCD_F16_FWD(scd_bn_bwd_reduce, dout, mask, y, relu_scale, relu_shift, mean, invstd, C, total, stats, stream);
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return launch_bwd_reduce<T, 1>({(const T*)dout, (const T*)mask, {(const T*)y}, relu_scale, relu_shift,
                                        {mean, invstd}, C, 0, 0, 0, {stats}}, total, stream);
    });
}

extern "C" int scd_bn_bwd_reduce2(int dtype, const void* dout, const void* mask, const void* ya, const void* yb,
                                  const float* mean_a, const float* invstd_a, const float* mean_b,
                                  const float* invstd_b, int C, long total, double* stats_a, double* stats_b,
                                  void* stream) {
    SCD_F16_FWD(scd_bn_bwd_reduce2, dout, mask, ya, yb, mean_a, invstd_a, mean_b, invstd_b, C, total, stats_a, stats_b,
                stream);
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (!dout || !mask || !ya || !yb) return SCD_ERR_ARG;
        return launch_bwd_reduce<T, 2>({(const T*)dout, (const T*)mask, {(const T*)ya, (const T*)yb},
                                        {mean_a, invstd_a, mean_b, invstd_b}, C, 0, 0, 0, {stats_a, stats_b}}, total,
                                       stream);
    });
}

extern "C" int scd_bn_bwd_apply2(int dtype, const void* dout, const void* mask, const void* ya, const void* yb,
                                 const float* coef_a, const float* coef_b, int C, long total, void* dya, void* dyb,
                                 void* stream) {
    SCD_F16_FWD(scd_bn_bwd_apply2, dout, mask, ya, yb, coef_a, coef_b, C, total, dya, dyb, stream);
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        constexpr int E = 16 / sizeof(T);
        if (!dout || !mask || !ya || !yb || !dya || !dyb || total / E >= (1L << 32)) return SCD_ERR_ARG;
        return launch_bwd_apply<T, 2>({(const T*)dout, (const T*)mask, {(const T*)ya, (const T*)yb}, {coef_a, coef_b},
                                       C, 0, {(T*)dya, (T*)dyb}}, total, stream);
    });
}

extern "C" int scd_bn_bwd_apply(int dtype, const void* dout, const void* mask, const void* y, const float* relu_scale,
                                const float* relu_shift, const float* coef, int C, long total, void* dy, void* dz,
                                void* stream) {
    SCD_F16_FWD(scd_bn_bwd_apply, dout, mask, y, relu_scale, relu_shift, coef, C, total, dy, dz, stream);
    return scd_dispatch_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return launch_bwd_apply<T, 1>({(const T*)dout, (const T*)mask, {(const T*)y}, relu_scale, relu_shift, {coef}, C,
                                       0, {(T*)dy}, (T*)dz}, total, stream);
    });
}

// ---------------------------------------------------------------- statistics: collapse and finalize (no dtype)
// fp64 sums in, fp32 per-channel parameters out: the first build alone holds these entry points and their kernels.
#ifndef SCD_F16_BUILD
namespace {

// sum replicas into replica 0 and zero the others (buffers are persistent: the consumer re-zeroes)
__global__ void stats_collapse_kernel(double* stats, int nrep, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < nrep; ++r) {
        s += stats[(long)r * n + i];
        if (r) stats[(long)r * n + i] = 0.0;
    }
    stats[i] = s;
}

// SyncBN staging: out[i] = sum of the replicas, every replica zeroed (two layers' sums side by side in one buffer,
// so one collective reduces both)
__global__ void stats_collapse_to_kernel(double* stats, int nrep, int n, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < nrep; ++r) {
        s += stats[(long)r * n + i];
        stats[(long)r * n + i] = 0.0;
    }
    out[i] = s;
}

// one wave per channel: lane r sums replica r (and zeroes it: persistent, consumer-cleared buffers)
__device__ __forceinline__ void wave_collect(double* stats, int nrep, int C, int c, double& s, double& q) {
    const int lane = threadIdx.x & 63;
    double a = 0.0, b = 0.0;
    for (int r = lane; r < nrep; r += 64) {
        double* p = stats + (long)r * 2 * C;
        a += p[c];
        b += p[C + c];
        p[c] = 0.0;
        p[C + c] = 0.0;
    }
    s = wave_sum_d(a);
    q = wave_sum_d(b);
}

__device__ __forceinline__ void bn_finalize_channel(int c, double* stats, int nrep, int C, double count,
                                                    const float* gamma, const float* beta, float* rmean, float* rvar,
                                                    float momentum, float eps, float* mean_o, float* invstd_o,
                                                    float* scale_o, float* shift_o, int64_t* nbt) {
    double mean, var;
    if (stats) {
        double s, q;
        wave_collect(stats, nrep, C, c, s, q);
        mean = s / count;
        var = q / count - mean * mean;
        if (var < 0.0) var = 0.0;
    } else {                       // eval mode: normalise with the running statistics
        mean = rmean[c];
        var = rvar[c];
    }
    if ((threadIdx.x & 63) != 0) return;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float g = gamma ? gamma[c] : 1.f;
    const float b = beta ? beta[c] : 0.f;
    const float sc = g * invstd;
    mean_o[c] = (float)mean;
    invstd_o[c] = invstd;
    scale_o[c] = sc;
    shift_o[c] = b - (float)mean * sc;
    // (statistics that are NaN -- a failed peer-memory SyncBN all-reduce poisons its result, scdhip/peer.py -- leave the
    // running statistics AND num_batches_tracked as they were, so a checkpoint written after the failure still carries
    // the last good, mutually consistent ones; channel 0's lane counts the batch)
    if (c == 0 && nbt && stats && mean == mean && var == var) *nbt += 1;
    if (stats && rmean && mean == mean && var == var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
    }
}

// 1 .. SCD_BN_FIN_MAX layers in one launch (forward or backward finalize): layer i owns blocks [b0[i], b0[i + 1])
template <typename Args>
struct FinN {
    Args l[SCD_BN_FIN_MAX];
    int b0[SCD_BN_FIN_MAX + 1];
    int n;
};
// this block's layer, and this wave's channel c in it (one wave per channel, 4 per 256-thread block)
template <typename Args>
__device__ __forceinline__ const Args& fin_layer(const FinN<Args>& f, int& c) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < SCD_BN_FIN_MAX; ++k)
        if (k < f.n && (int)blockIdx.x >= f.b0[k]) i = k;
    const Args& a = f.l[i];
    c = (blockIdx.x - f.b0[i]) * (blockDim.x / 64) + (threadIdx.x >> 6);
    return a;
}
inline int fin_blocks(int C) { return (C + 3) / 4; }

__global__ void bn_finalize_n_kernel(FinN<scd_bn_fin_args> f) {
    int c;
    const scd_bn_fin_args& a = fin_layer(f, c);
    if (c >= a.C) return;
    bn_finalize_channel(c, a.stats, a.nrep, a.C, a.count, a.gamma, a.beta, a.running_mean, a.running_var, a.momentum,
                        a.eps, a.mean, a.invstd, a.scale, a.shift, a.num_batches);
}

__device__ __forceinline__ void bn_bwd_finalize_channel(int c, double* stats, int nrep, int C, double count,
                                                        const float* gamma, const float* mean, const float* invstd,
                                                        float* dgamma, float* dbeta, float gscale, float* coef) {
    double s, q;
    wave_collect(stats, nrep, C, c, s, q);
    if ((threadIdx.x & 63) != 0) return;
    if (dgamma) dgamma[c] += gscale * (float)q;
    if (dbeta) dbeta[c] += gscale * (float)s;
    const float g = gamma ? gamma[c] : 1.f;
    const float is = invstd[c];
    const float sc = g * is;
    const float k1 = (float)(s / count);
    const float k2 = (float)(q / count);
    // dy = sc*(dz - k1 - xhat*k2), xhat = (y-mean)*is
    coef[c] = sc;
    coef[C + c] = -sc * is * k2;
    coef[2 * C + c] = -sc * k1 + sc * is * k2 * mean[c];
}

// (kept beside the _n kernel: through the layer array a single layer's launch took 0.3 us longer at C = 2048)
__global__ void bn_bwd_finalize_kernel(double* stats, int nrep, int C, double count, const float* gamma,
                                       const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                       float gscale, float* coef) {
    const int c = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (c >= C) return;
    bn_bwd_finalize_channel(c, stats, nrep, C, count, gamma, mean, invstd, dgamma, dbeta, gscale, coef);
}

__global__ void bn_bwd_finalize_n_kernel(FinN<scd_bn_bwd_fin_args> f) {
    int c;
    const scd_bn_bwd_fin_args& a = fin_layer(f, c);
    if (c >= a.C) return;
    bn_bwd_finalize_channel(c, a.stats, a.nrep, a.C, a.count, a.gamma, a.mean, a.invstd, a.dgamma, a.dbeta, a.gscale,
                            a.coef);
}

// the launch of Kernel over layers[0 .. n), each of which passes the entry point's own test `ok`
template <auto Kernel, typename Args, typename Ok>
int launch_finalize_n(const Args* layers, int n, Ok ok, void* stream) {
    if (!layers || n < 1 || n > SCD_BN_FIN_MAX) return SCD_ERR_ARG;
    FinN<Args> f;
    memset(&f, 0, sizeof(f));
    f.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (!ok(layers[i])) return SCD_ERR_ARG;
        f.l[i] = layers[i];
        f.b0[i] = blocks;
        blocks += fin_blocks(layers[i].C);
    }
    f.b0[n] = blocks;
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, f);
    SCD_RETURN_LAUNCH();
}

}  // namespace

extern "C" int scd_stats_collapse(double* stats, int nrep, int C, void* stream) {
    const int n = 2 * C;
    hipLaunchKernelGGL(stats_collapse_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, stats, nrep, n);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_stats_collapse_to(double* stats, int nrep, int C, double* out, void* stream) {
    const int n = 2 * C;
    if (!stats || !out || nrep < 1) return SCD_ERR_ARG;
    hipLaunchKernelGGL(stats_collapse_to_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, stats, nrep, n,
                       out);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_bn_finalize(double* stats, int nrep, int C, double count, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, int64_t* num_batches,
                               float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                               void* stream) {
    const scd_bn_fin_args layer = {stats, nrep, C, count, gamma, beta, running_mean, running_var, num_batches,
                                   momentum, eps, mean, invstd, scale, shift};
    return scd_bn_finalize_n(&layer, 1, stream);
}

extern "C" int scd_bn_finalize_n(const scd_bn_fin_args* layers, int n, void* stream) {
    return launch_finalize_n<bn_finalize_n_kernel>(layers, n, [](const scd_bn_fin_args& l) { return l.C > 0; },
                                                   stream);
}

extern "C" int scd_bn_bwd_finalize_n(const scd_bn_bwd_fin_args* layers, int n, void* stream) {
    return launch_finalize_n<bn_bwd_finalize_n_kernel>(
        layers, n,
        [](const scd_bn_bwd_fin_args& l) { return l.C > 0 && l.stats && l.invstd && l.mean && l.coef; }, stream);
}

extern "C" int scd_bn_bwd_finalize(double* stats, int nrep, int C, double count, const float* gamma,
                                   const float* mean, const float* invstd, float* dgamma, float* dbeta, float gscale,
                                   float* coef, void* stream) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(fin_blocks(C)), dim3(256), 0, (hipStream_t)stream, stats, nrep, C,
                       count, gamma, mean, invstd, dgamma, dbeta, gscale, coef);
    SCD_RETURN_LAUNCH();
}
#endif  // !SCD_F16_BUILD
