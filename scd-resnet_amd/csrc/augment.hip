// SCD tile augmentation on the GPU (the sample half; the target half is targets.hip).
//
// Reference: datasets/scds/scdx16p100.py:416-441 (SCD.argumentation: random x / y flips, then normalize,
// varianceJitter, gaussianNoise) and datasets/argumentations.py:38-64:
//   normalize:      mean = mean(t); var = mean((t - mean)^2); t = (t - mean) / sqrt(var)
//   varianceJitter: t * (1 + 0.05 * g),  g ~ N(0,1) one draw per tile
//   gaussianNoise:  t + n * 0.05,        n ~ N(0,1) per pixel
// The validation set uses normalize alone (scdx16p100.py:216).
//
// Two launches per batch: (1) per-(tile, slice) fp64 partial sums of x and x^2 into the caller's workspace
// (deterministic: no atomics); (2) every block re-reduces its tile's partials (64 values), derives mean and
// variance in fp64, and writes the flipped, normalised, jittered, noised tile with float4 loads / stores.
// Per-pixel noise comes from the caller (a device tensor: parity tests replay the reference's draws) or from
// a counter-based generator (splitmix64 of (seed, tile, pixel) -> Box-Muller), so the batch path needs no
// host random numbers.
// scd_augment_tiles_indexed runs the same two kernels on tiles ids[b] of a device-resident store, read in place.
//
// scd_rotate_tiles: the per-sample random rotation the reference wrote as the last step of SCD.argumentation and left
// switched off (scdx16p100.py:443-451): out[b] = argumentations.rotate(in[b], angle_b, MirrorPadding, Bilinear)
// (argumentations.py:148-159: torch-'reflect' padding to the diagonal, torchvision's tensor rotate about the padded
// frame's centre, the centre crop) in one launch that materialises neither the padded nor the rotated frame -- the
// arithmetic of preprocess.hip's slide rotation (rotate_taps.h) with a single reflection and one angle per tile.
#include "rotate_taps.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_SLICES = 64;
constexpr int AUG_THREADS = 256;

// Tile b of a batch is tile ids[b] of `in` (scd_augment_tiles_indexed: a gather from a device-resident store, read in
// place by both passes) or, with ids NULL, tile b itself (scd_augment_tiles).  The offset is 64-bit: the canonical
// store holds 1.3e10 elements.
__device__ __forceinline__ const float* aug_tile(const float* in, const int* ids, int b, long hw) {
    return in + (long)(ids ? ids[b] : b) * hw;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_stats_kernel(const float* __restrict__ in,
                                                                const int* __restrict__ ids, long hw,
                                                                double* __restrict__ part) {
    const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    const long n4 = hw >> 2;
    const long per = (n4 + AUG_SLICES - 1) / AUG_SLICES;
    const long beg = s * per, end = min(n4, beg + per);
    const float4* p = (const float4*)aug_tile(in, ids, b, hw);
    double s1 = 0.0, s2 = 0.0;
    for (long i = beg + tid; i < end; i += AUG_THREADS) {
        float4 v = p[i];
        s1 += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
        s2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    if (block_sums_d<AUG_THREADS / 64>(s1, s2, AUG_THREADS / 64)) {
        part[((long)b * AUG_SLICES + s) * 2] = s1;
        part[((long)b * AUG_SLICES + s) * 2 + 1] = s2;
    }
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// two N(0,1) values per 64-bit draw (Box-Muller on two 24-bit uniforms in (0,1])
__device__ __forceinline__ float2 gauss2(unsigned long long seed, unsigned long long ctr) {
    unsigned long long r = splitmix64(seed ^ splitmix64(ctr));
    float u1 = ((float)(r & 0xffffffu) + 1.f) * (1.f / 16777216.f);
    float u2 = (float)((r >> 24) & 0xffffffu) * (1.f / 16777216.f);
    float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    return make_float2(rad * cs, rad * sn);
}

struct AugArgs {
    const float* in;
    const int* ids;          // (B) tile of `in` per batch slot, nullable = identity
    float* out;
    const double* part;
    const uint8_t* flips;    // (B,2): [flip x (dim 2), flip y (dim 1)]
    const float* jitter;     // (B): the factor (1 + 0.05 g), nullable = 1
    const float* noise;      // (B,H,W) N(0,1) draws, nullable -> counter-based generator
    float noise_sv;          // 0 disables the noise term
    unsigned long long seed;
    int H, W;
};

__global__ __launch_bounds__(AUG_THREADS) void aug_apply_kernel(AugArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long hw = (long)a.H * a.W;
    __shared__ float coef[2];
    if (tid < 64) {
        double s1 = a.part[((long)b * AUG_SLICES + tid) * 2], s2 = a.part[((long)b * AUG_SLICES + tid) * 2 + 1];
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        if (tid == 0) {
            double mean = s1 / (double)hw;
            double var = s2 / (double)hw - mean * mean;
            coef[0] = (float)mean;
            coef[1] = __fsqrt_rn((float)(var > 0.0 ? var : 0.0));
        }
    }
    __syncthreads();
    const float mean = coef[0], sd = coef[1];
    const float jit = a.jitter ? a.jitter[b] : 1.f;
    const bool fx = a.flips && a.flips[b * 2], fy = a.flips && a.flips[b * 2 + 1];
    const int w4 = a.W >> 2;
    const long n4 = hw >> 2;
    const float* src = aug_tile(a.in, a.ids, b, hw);
    float* dst = a.out + (long)b * hw;
    for (long i = (long)blockIdx.x * AUG_THREADS + tid; i < n4; i += (long)gridDim.x * AUG_THREADS) {
        int y = (int)(i / w4), x4 = (int)(i - (long)y * w4);
        int sy = fy ? a.H - 1 - y : y;
        int sx4 = fx ? w4 - 1 - x4 : x4;
        float4 v = *(const float4*)(src + (long)sy * a.W + sx4 * 4);
        if (fx) v = make_float4(v.w, v.z, v.y, v.x);
        float r[4] = {v.x, v.y, v.z, v.w};
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.noise_sv != 0.f) {
            if (a.noise) {
                float4 q = *(const float4*)(a.noise + (long)b * hw + i * 4);
                nz[0] = q.x; nz[1] = q.y; nz[2] = q.z; nz[3] = q.w;
            } else {
                unsigned long long ctr = ((unsigned long long)b << 40) + (unsigned long long)i * 2;
                float2 g0 = gauss2(a.seed, ctr), g1 = gauss2(a.seed, ctr + 1);
                nz[0] = g0.x; nz[1] = g0.y; nz[2] = g1.x; nz[3] = g1.y;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = __fdiv_rn(__fsub_rn(r[j], mean), sd);
            t = __fmul_rn(t, jit);
            r[j] = __fadd_rn(t, __fmul_rn(nz[j], a.noise_sv));
        }
        *(float4*)(dst + i * 4) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

struct RotTiles {
    const float* in;
    float* out;
    const double* cs;       // (B,2): cos, sin of each tile's angle
    int B, H, W;
    int lp, tp;             // rotate()'s diagonal padding
    long units;             // workgroup footprints per tile
};

// One thread = four adjacent output pixels.  The 256 threads of a workgroup cover a footprint of PW quads x 256 / PW
// rows (PW = 1 << LOGPW), so a wave covers 4 PW pixels x 64 / PW rows; LOGPW < 0: 256 consecutive quads of the
// flattened tile (a wave = 256 pixels of one row when W >= 256).  Footprints stride over grid.x, tiles over grid.y.
template <int LOGPW>
__global__ __launch_bounds__(AUG_THREADS) void rotate_tiles_kernel(RotTiles a) {
    const int tid = threadIdx.x;
    const int w4 = a.W >> 2;
    const int Wq = a.W + 2 * a.lp, Hq = a.H + 2 * a.tp;
    const double mx = 0.5 * (double)(Wq - 1), my = 0.5 * (double)(Hq - 1);
    const long hw = (long)a.H * a.W;
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const double ca = a.cs[(long)b * 2], sa = a.cs[(long)b * 2 + 1];
        const float* src = a.in + (long)b * hw;
        float* dst = a.out + (long)b * hw;
        for (long u = blockIdx.x; u < a.units; u += gridDim.x) {
            int i, q;
            if (LOGPW < 0) {
                const long e = u * AUG_THREADS + tid;
                i = (int)(e / w4);
                q = (int)(e - (long)i * w4);
            } else {
                constexpr int LW = LOGPW < 0 ? 0 : LOGPW, PW = 1 << LW, PH = AUG_THREADS >> LW;
                const int ux = (w4 + PW - 1) >> LW;
                const long uy = u / ux;
                i = (int)uy * PH + (tid >> LW);
                q = (int)(u - uy * ux) * PW + (tid & (PW - 1));
            }
            if (i >= a.H || q >= w4) continue;
            const double yc = (double)(i + a.tp) - my;
            float res[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double xc = (double)(q * 4 + k + a.lp) - mx;
                const double sx = (ca * xc - sa * yc) + mx;
                const double sy = (sa * xc + ca * yc) + my;
                int x0, y0;
                float wx, wy;
                rot_cell(sx, sy, x0, y0, wx, wy);
                // taps outside the padded frame are grid_sample's zeros; inside it, -W < tap - lp < 2W - 1 as lp < W
                const bool cin0 = x0 >= 0 && x0 < Wq, cin1 = x0 + 1 >= 0 && x0 + 1 < Wq;
                const bool rin0 = y0 >= 0 && y0 < Hq, rin1 = y0 + 1 >= 0 && y0 + 1 < Hq;
                const int c0 = cin0 ? reflect_idx(x0 - a.lp, a.W) : 0, c1 = cin1 ? reflect_idx(x0 + 1 - a.lp, a.W) : 0;
                const long r0 = (long)(rin0 ? reflect_idx(y0 - a.tp, a.H) : 0) * a.W;
                const long r1 = (long)(rin1 ? reflect_idx(y0 + 1 - a.tp, a.H) : 0) * a.W;
                const float v00 = rin0 && cin0 ? src[r0 + c0] : 0.0f, v01 = rin0 && cin1 ? src[r0 + c1] : 0.0f;
                const float v10 = rin1 && cin0 ? src[r1 + c0] : 0.0f, v11 = rin1 && cin1 ? src[r1 + c1] : 0.0f;
                res[k] = rot_lerp(v00, v01, v10, v11, wx, wy);
            }
            *(float4*)(dst + (long)i * a.W + q * 4) = make_float4(res[0], res[1], res[2], res[3]);
        }
    }
}

template <int LOGPW>
int rotate_tiles_launch(RotTiles a, hipStream_t st) {
    if (LOGPW < 0) {
        a.units = ((long)a.H * (a.W >> 2) + AUG_THREADS - 1) / AUG_THREADS;
    } else {
        constexpr int LW = LOGPW < 0 ? 0 : LOGPW, PW = 1 << LW, PH = AUG_THREADS >> LW;
        a.units = (long)(((a.W >> 2) + PW - 1) / PW) * ((a.H + PH - 1) / PH);
    }
    const dim3 grid((unsigned)min(a.units, 1L << 20), (unsigned)min(a.B, 65535));
    hipLaunchKernelGGL(rotate_tiles_kernel<LOGPW>, grid, dim3(AUG_THREADS), 0, st, a);
    SCD_RETURN_LAUNCH();
}

}  // namespace

extern "C" size_t scd_augment_workspace(int B) { return (size_t)B * AUG_SLICES * 2 * sizeof(double); }

// the two launches of both entry points: ids NULL = identity indexing
static int augment_launch(const float* in, const int* ids, float* out, int B, int H, int W, const uint8_t* flips,
                          const float* jitter, const float* noise, float noise_sv, unsigned long long seed,
                          void* workspace, void* stream) {
    if (B < 1 || H < 1 || W < 4 || (W & 3) || (long)H * W >= (1L << 31) || in == out) return SCD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)H * W;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(aug_stats_kernel, dim3(AUG_SLICES, B), dim3(AUG_THREADS), 0, st, in, ids, hw, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    AugArgs a{in, ids, out, part, flips, jitter, noise, noise_sv, seed, H, W};
    int bx = (int)min(64L, (hw / 4 + AUG_THREADS - 1) / AUG_THREADS);
    hipLaunchKernelGGL(aug_apply_kernel, dim3(bx, B), dim3(AUG_THREADS), 0, st, a);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_augment_tiles(const float* in, float* out, int B, int H, int W, const uint8_t* flips,
                                 const float* jitter, const float* noise, float noise_sv, unsigned long long seed,
                                 void* workspace, void* stream) {
    return augment_launch(in, nullptr, out, B, H, W, flips, jitter, noise, noise_sv, seed, workspace, stream);
}

extern "C" int scd_augment_tiles_indexed(const float* store, long nstore, const int* ids, float* out, int B, int H,
                                         int W, const uint8_t* flips, const float* jitter, const float* noise,
                                         float noise_sv, unsigned long long seed, void* workspace, void* stream) {
    if (!store || !ids || !out || nstore < 1) return SCD_ERR_ARG;
    return augment_launch(store, ids, out, B, H, W, flips, jitter, noise, noise_sv, seed, workspace, stream);
}

extern "C" int scd_rotate_tiles_mapped(const float* in, float* out, int B, int H, int W, const double* cs, int mapping,
                                       void* stream) {
    if (!in || !out || !cs || in == out || B < 1 || H < 2 || W < 4 || (W & 3) || (long)H * W >= (1L << 31))
        return SCD_ERR_ARG;
    const double radius = sqrt((double)W * W + (double)H * H) / 2.0;           // argumentations.py:153-155
    const long lp = (long)ceil(radius - 0.5 * W), tp = (long)ceil(radius - 0.5 * H);
    if (lp >= W || tp >= H) return SCD_ERR_ARG;                                // 'reflect' needs pad < size
    const RotTiles a{in, out, cs, B, H, W, (int)lp, (int)tp, 0};
    hipStream_t st = (hipStream_t)stream;
    switch (mapping) {
        case SCD_ROTATE_MAP_ROW: return rotate_tiles_launch<-1>(a, st);
        case SCD_ROTATE_MAP_64X4: return rotate_tiles_launch<4>(a, st);
        case SCD_ROTATE_MAP_32X8: return rotate_tiles_launch<3>(a, st);
        case SCD_ROTATE_MAP_16X16: return rotate_tiles_launch<2>(a, st);
    }
    return SCD_ERR_ARG;
}

extern "C" int scd_rotate_tiles(const float* in, float* out, int B, int H, int W, const double* cs, void* stream) {
    return scd_rotate_tiles_mapped(in, out, B, H, W, cs, SCD_ROTATE_MAP_DEFAULT, stream);
}
