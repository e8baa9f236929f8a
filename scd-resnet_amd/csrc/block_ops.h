// What the loss, decode and data-path kernels share (api, loss_decode, targets, slide, augment, preprocess; the GEMM
// files do not include this header): the workgroup sum of fp64 partials, the ordered compaction step, the focal
// element terms, the k x k NMS kernel, torch's 'reflect' index and the element-wise grid.  No `fp contract` pragma
// here: the floating-point pieces (focal, NMS) exist only for a file that defines BLOCK_OPS_FP before the include --
// api.hip and loss_decode.hip, which compile with the default contraction; the files that switch it off take the
// integer and fp64-addition helpers, which have nothing to contract.
#pragma once
#include <algorithm>

#include "scd_common.h"

// grid of a 256-thread element-wise kernel with a grid-stride loop
static inline int ew_blocks(long n) { return (int)std::min<long>(4096, std::max<long>(1, (n + 255) / 256)); }

// torch 'reflect' (no edge repeat); valid for -n < i < 2n - 1
__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// Workgroup sums of two or three doubles over nw <= MAXW waves: wave_sum_d per value, one LDS slot per wave, then
// thread 0 adds the waves in ascending wave index -- fp64 addition is not associative, and this order is what keeps
// every sum bit-identical.  True on thread 0 alone, where the arguments then hold the sums; what becomes of them (a
// partial slot, an atomic_add_f64 to a replica slot, a finalize) is the caller's.  One barrier; once per kernel (its
// own LDS).  (Written on scalars: over an array of values the shuffle chains came out in another order.)
template <int MAXW>
__device__ __forceinline__ bool block_sums_d(double& a, double& b, int nw) {
    __shared__ double red[2][MAXW];
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < nw; ++k) { s0 += red[0][k]; s1 += red[1][k]; }
        a = s0;
        b = s1;
    }
    return threadIdx.x == 0;
}
template <int MAXW>
__device__ __forceinline__ bool block_sums_d(double& a, double& b, double& c, int nw) {
    __shared__ double red[3][MAXW];
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    c = wave_sum_d(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = a; red[1][w] = b; red[2][w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nw; ++k) { s0 += red[0][k]; s1 += red[1][k]; s2 += red[2][k]; }
        a = s0;
        b = s1;
        c = s2;
    }
    return threadIdx.x == 0;
}

// Ordered compaction over a workgroup of nw <= MAXW waves, one chunk of blockDim elements per step: the kept elements
// of all steps get consecutive offsets in thread order.  `base` (zeroed by the caller, behind a barrier) is the running
// count, uniform and current on return; the scratch is the caller's so that a kernel with two compactions pays it once.
template <int MAXW>
struct CompactLds {
    int wtot[MAXW];
    int base;
};

template <int MAXW>
__device__ __forceinline__ int block_compact(bool keep, CompactLds<MAXW>& s, int nw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s.wtot[wv] = __popcll(bal);
    __syncthreads();
    int off = s.base + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) off += s.wtot[w];
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < nw; ++w) t += s.wtot[w];
        s.base += t;
    }
    __syncthreads();
    return off;
}

// A second count beside a compaction (an integer, so exact in any order): the workgroup's lanes with `flag` set, added
// to an LDS counter; the barriers of the block_compact that follows order it before any read.
__device__ __forceinline__ void block_count(bool flag, int* counter) {
    const unsigned long long bal = __ballot(flag);
    if ((threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(bal));
}

// ---- the floating-point pieces: only for a file that compiles with the default contraction and says so
#ifdef BLOCK_OPS_FP
namespace {

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

constexpr int FOCAL_ACC = 4;     // posL, negL, npos, pad: one replica slot of a focal accumulator

// focal.py:25-53 on a probability pc with target t: the element's term added to posl / negl / npos, d = dL/dp up to
// the normaliser.  The sums go in and come back by value: with reference parameters here the compiler simplifies the
// branches before it inlines them and then forms other FMAs than in the kernels this came from, and the gradients
// change in the last bit.  (Only this shape of the code pins the contraction: a compiler change can move it.)
struct FocalStep {
    float d, posl, negl, npos;
};
__device__ __forceinline__ FocalStep focal_step(float pc, float t, float posl, float negl, float npos) {
    float dterm = 0.f;
    if (t == 1.f) {
        const float om = 1.f - pc;
        const float lg = logf(pc);
        posl += lg * (om * om);
        npos += 1.f;
        dterm = om * om / pc - 2.f * om * lg;
    } else if (t < 1.f) {
        const float om = 1.f - t;
        const float w = (om * om) * (om * om);
        const float l1m = logf(1.f - pc);
        negl += l1m * (pc * pc) * w;
        dterm = w * (-(pc * pc) / (1.f - pc) + 2.f * pc * l1m);
    }
    return FocalStep{dterm, posl, negl, npos};
}
// the caller's form: updates the three sums, returns d
__device__ __forceinline__ float focal_term(float pc, float t, float& posl, float& negl, float& npos) {
    const FocalStep r = focal_step(pc, t, posl, negl, npos);
    posl = r.posl; negl = r.negl; npos = r.npos;
    return r.d;
}

// the same on a logit: sigmoid, clamp to [1e-4, 1 - 1e-4]; returns dL/dlogit, 0 where the clamp holds the probability
__device__ __forceinline__ float focal_logit_term(float xi, float t, float& posl, float& negl, float& npos) {
    const float p = sigmoid_f(xi);
    const bool pass = (p >= 1e-4f) && (p <= 1.f - 1e-4f);
    const float pc = fminf(fmaxf(p, 1e-4f), 1.f - 1e-4f);
    const float dterm = focal_term(pc, t, posl, negl, npos);
    return pass ? dterm * p * (1.f - p) : 0.f;
}

// a workgroup's focal sums into its replica slot of acc (256 threads)
__device__ __forceinline__ void focal_accumulate(float posl, float negl, float npos, double* acc) {
    double a = (double)posl, b = (double)negl, c = (double)npos;
    if (block_sums_d<4>(a, b, c, blockDim.x / 64)) {
        double* dst = acc + (long)(blockIdx.x % SCD_STAT_REPLICAS) * FOCAL_ACC;
        atomic_add_f64(dst + 0, a);
        atomic_add_f64(dst + 1, b);
        atomic_add_f64(dst + 2, c);
    }
}

// out = V::value(x) where it equals its k x k neighbourhood max (padding -inf), else 0 -- heat * (maxpool(heat) ==
// heat), utility.py:87-92.  NmsProduct forms that product on x itself (a NaN stays NaN, as in torch); NmsSigmoid is the
// decode's: the map of sigmoid(x), a non-peak (or NaN) pixel exactly 0.
struct NmsProduct {
    __device__ static float value(float x) { return x; }
    __device__ static float keep(float v, bool peak) { return v * (peak ? 1.f : 0.f); }
};
struct NmsSigmoid {
    __device__ static float value(float x) { return sigmoid_f(x); }
    __device__ static float keep(float v, bool peak) { return peak ? v : 0.f; }
};

template <typename V>
__global__ void nms_kernel(const float* x, long planes, int H, int W, int k, float* out) {
    const long total = planes * H * W;
    const int r = (k - 1) / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long pl = i / ((long)H * W);
        const int rem = (int)(i - pl * H * W);
        const int y = rem / W, xx = rem - (rem / W) * W;
        const float* hp = x + pl * H * W;
        const float v = V::value(hp[rem]);
        float m = -INFINITY;
        for (int dy = -r; dy <= k - 1 - r; ++dy) {
            const int yy = y + dy;
            if ((unsigned)yy >= (unsigned)H) continue;
            for (int dx = -r; dx <= k - 1 - r; ++dx) {
                const int xc = xx + dx;
                if ((unsigned)xc >= (unsigned)W) continue;
                m = fmaxf(m, V::value(hp[yy * W + xc]));
            }
        }
        out[i] = V::keep(v, m == v);
    }
}

}  // namespace
#endif
