// Whole-slide tiled inference on the GPU.
//
// Reference: test.py:19-32 (grayscale: round(0.1140 c0 + 0.5870 c1 + 0.2989 c2) in float64), :38-87 (resize to
// whole 384-px strides + 2 x 64 margin, torch 'reflect' padding, then the opencv-style column fix-up:
// col[x] = col[127 - x] for x < 64 and col[x] = col[6271 - x] for 3136 <= x < 3200, clips of 512 x 512 taken
// x-major, each normalised in float64 and cast to float32), :90-135 (score > 0.3, detections projected back:
// (int(x * 384 - padLR + cx * 4 + offx), int(y * 384 - padTB + cy * 4 + offy), ratio = (4 halo - 4 minl) /
// (2 * 4 minl))).
//
// scd_slide_tiles: two launches.  (1) per (tile, slice) exact fp64 sums of the grey values (integers
// 0..255, so every sum is exact) read straight from the RGB slide through the padding / fix-up index map;
// (2) normalise: (g - mean) / sqrt(var) in float64, stored as float32 (B,1,512,512).  No padded slide is
// materialised.  scd_slide_detections: one workgroup walks the decoded (10, T, K) stack tile by tile,
// compacting the kept detections in the reference's order with wave ballots.  scd_slide_samples (the end of the
// file): the box filter, cross-clip de-duplication and Rhr histogram of test.py:148-183.
#include "block_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int SL_SLICES = 32;
constexpr int SL_THREADS = 256;

struct SlideGeom {
    const uint8_t* rgb;     // (H, W, C) interleaved, C >= 3
    int H, W, C;
    int tile, stride;       // 512, 384
    int clipH, clipV;       // tiles along x, along y
    int padLR, padTB;
    int resizeW;
    int fix;                // apply the opencv column fix-up (test.py:79-82)
};

// grey value of padded pixel (py, px)
__device__ __forceinline__ double grey_at(const SlideGeom& g, int py, int px) {
    if (g.fix) {
        if (px < 64) px = 127 - px;
        else if (px >= 3136 && px < 3200) px = 6271 - px;
    }
    int sy = reflect_idx(py - g.padTB, g.H), sx = reflect_idx(px - g.padLR, g.W);
    const uint8_t* p = g.rgb + ((long)sy * g.W + sx) * g.C;
    double v = 0.1140 * (double)p[0] + 0.5870 * (double)p[1];
    v = v + 0.2989 * (double)p[2];
    return rint(v);
}

__device__ __forceinline__ void tile_origin(const SlideGeom& g, int t, int& oy, int& ox) {
    int i = t / g.clipV, j = t - (t / g.clipV) * g.clipV;   // x-major (test.py:84-87)
    ox = i * g.stride;
    oy = j * g.stride;
}

__global__ __launch_bounds__(SL_THREADS) void slide_stats_kernel(SlideGeom g, double* part) {
    const int t = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    int oy, ox;
    tile_origin(g, t, oy, ox);
    const int rows = (g.tile + SL_SLICES - 1) / SL_SLICES;
    double s1 = 0.0, s2 = 0.0;
    for (int r = s * rows; r < min(g.tile, (s + 1) * rows); ++r)
        for (int c = tid; c < g.tile; c += SL_THREADS) {
            double v = grey_at(g, oy + r, ox + c);
            s1 += v;
            s2 += v * v;
        }
    if (block_sums_d<SL_THREADS / 64>(s1, s2, SL_THREADS / 64)) {
        part[((long)t * SL_SLICES + s) * 2] = s1;
        part[((long)t * SL_SLICES + s) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(SL_THREADS) void slide_apply_kernel(SlideGeom g, const double* part, float* out) {
    const int t = blockIdx.y, tid = threadIdx.x;
    __shared__ double coef[2];
    if (tid < 64) {
        double a = tid < SL_SLICES ? part[((long)t * SL_SLICES + tid) * 2] : 0.0;
        double b = tid < SL_SLICES ? part[((long)t * SL_SLICES + tid) * 2 + 1] : 0.0;
        a = wave_sum_d(a);
        b = wave_sum_d(b);
        if (tid == 0) {
            double n = (double)g.tile * g.tile;
            double mean = a / n;
            coef[0] = mean;
            coef[1] = sqrt(b / n - mean * mean);
        }
    }
    __syncthreads();
    const double mean = coef[0], sd = coef[1];
    int oy, ox;
    tile_origin(g, t, oy, ox);
    const long n = (long)g.tile * g.tile;
    float* dst = out + (long)t * n;
    for (long i = (long)blockIdx.x * SL_THREADS + tid; i < n; i += (long)gridDim.x * SL_THREADS) {
        int r = (int)(i / g.tile), c = (int)(i - (long)r * g.tile);
        dst[i] = (float)((grey_at(g, oy + r, ox + c) - mean) / sd);
    }
}

// decoded stack rows (Wrapper order, trainer/wrappers/centerOffsetResidual.py:10-23):
// 0 scores, 1 inds, 2 ys, 3 xs, 4 majx, 5 majy, 6 minl, 7 halo, 8 offx, 9 offy
// Slot q = t*K + k projected back to slide pixels, and its ratio (test.py:124-137), in float64
__device__ __forceinline__ void slide_project(const float* dec, long plane, long q, int K, int stride, int padLR,
                                              int padTB, int clipV, int& px, int& py, double& rt) {
    int t = (int)(q / K);
    int i = t / clipV, j = t - (t / clipV) * clipV;
    double cx = dec[3 * plane + q], cy = dec[2 * plane + q];
    double ofx = dec[8 * plane + q], ofy = dec[9 * plane + q];
    px = (int)((double)(i * stride - padLR) + cx * 4.0 + ofx);
    py = (int)((double)(j * stride - padTB) + cy * 4.0 + ofy);
    double minl = (double)dec[6 * plane + q] * 4.0, halo = (double)dec[7 * plane + q] * 4.0;
    rt = (halo - minl) / (2.0 * minl);
}

// (block_compact written out: through the helper this kernel took 2 more instructions and one more VGPR)
__global__ __launch_bounds__(1024) void slide_detect_kernel(const float* dec, int T, int K, int stride, int padLR,
                                                            int padTB, int clipV, float thr, int* xy, double* ratio,
                                                            int* count) {
    __shared__ int wtot[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long plane = (long)T * K;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (long c0 = 0; c0 < plane; c0 += 1024) {
        long q = c0 + tid;
        bool keep = false;
        int px = 0, py = 0;
        double rt = 0.0;
        if (q < plane) {
            keep = dec[q] > thr;
            slide_project(dec, plane, q, K, stride, padLR, padTB, clipV, px, py, rt);
        }
        unsigned long long bal = __ballot(keep);
        int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wv] = __popcll(bal);
        __syncthreads();
        if (keep) {
            int off = base_s + rank;
            for (int w = 0; w < wv; ++w) off += wtot[w];
            xy[2 * off] = px;
            xy[2 * off + 1] = py;
            ratio[off] = rt;
        }
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int w = 0; w < 16; ++w) s += wtot[w];
            base_s += s;
        }
        __syncthreads();
    }
    if (tid == 0) *count = base_s;
}

}  // namespace

extern "C" size_t scd_slide_workspace(int ntiles) { return (size_t)ntiles * SL_SLICES * 2 * sizeof(double); }

extern "C" int scd_slide_tiles(const uint8_t* rgb, int H, int W, int C, int tile, int stride, int clipH, int clipV,
                               int padLR, int padTB, int fix, float* out, void* workspace, void* stream) {
    if (H < 2 || W < 2 || C < 3 || tile < 1 || stride < 1 || clipH < 1 || clipV < 1 || padLR < 0 || padTB < 0 ||
        padLR >= W || padTB >= H || (long)tile * tile >= (1L << 31))
        return SCD_ERR_ARG;
    const int resizeW = (clipH - 1) * stride + tile, resizeH = (clipV - 1) * stride + tile;
    if (resizeW > W + 2 * padLR || resizeH > H + 2 * padTB) return SCD_ERR_ARG;
    if (fix && resizeW < 3200) return SCD_ERR_ARG;   // the reference's fix-up indexes columns up to 3199
    SlideGeom g{rgb, H, W, C, tile, stride, clipH, clipV, padLR, padTB, resizeW, fix};
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    const int T = clipH * clipV;
    hipLaunchKernelGGL(slide_stats_kernel, dim3(SL_SLICES, T), dim3(SL_THREADS), 0, st, g, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(slide_apply_kernel, dim3(64, T), dim3(SL_THREADS), 0, st, g, (const double*)part, out);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_slide_detections(const float* decoded, int T, int K, int stride, int padLR, int padTB, int clipV,
                                    float thr, int* xy, double* ratio, int* count, void* stream) {
    if (T < 1 || K < 1 || clipV < 1 || (long)T * K >= (1L << 31)) return SCD_ERR_ARG;
    hipLaunchKernelGGL(slide_detect_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, decoded, T, K, stride, padLR,
                       padTB, clipV, thr, xy, ratio, count);
    SCD_RETURN_LAUNCH();
}

// ---- slide cohort quantification: scd_slide_samples ----
// Candidates (score > thr, pixel in the validity box) are compacted in flat order t*K + k, ranked by (score
// descending, flat index ascending) by counting, and de-duplicated greedily: a candidate is dropped when an
// already-kept candidate of another clip lies within `radius` pixels (integer dx^2 + dy^2 <= radius^2).  The pairs
// are tested once, in parallel, into a bit matrix in rank order (row = candidate, bit = a higher-ranked candidate
// that would suppress it if kept), stored as [row chunk][word][lane] so that the resolving workgroup reads it
// coalesced; one workgroup then walks the chunks in rank order, 64 rows at a time: the words of earlier chunks
// are ANDed against the kept bits by 16 waves, the diagonal word is resolved serially by wave 0.  The kept
// samples leave in flat order (the reference's), with the Rhr histogram built by LDS atomics and flushed once.
namespace {

constexpr int SS_CAP = SCD_SLIDE_SAMPLES_MAX;   // T*K slots
constexpr int SS_MAXBINS = 1024;
constexpr int SS_HDR = 16;                      // ints in front of the workspace: [0] candidates, [1] above thr

struct SamplesWs {
    int* hdr;
    double* cratio;
    int *cflat, *cpx, *cpy;
    float* cscore;
    int *rank, *spx, *spy, *sclip;
    unsigned long long* mat;
};

static inline size_t samples_ws_bytes(long plane) {
    long chunks = (plane + 63) / 64;
    return SS_HDR * sizeof(int) + (size_t)plane * (sizeof(double) + 8 * sizeof(int)) +
           (size_t)chunks * chunks * 64 * sizeof(unsigned long long);
}

static inline SamplesWs samples_ws(void* workspace, long plane) {
    SamplesWs w;
    char* p = (char*)workspace;
    w.hdr = (int*)p;                p += SS_HDR * sizeof(int);
    w.cratio = (double*)p;          p += plane * sizeof(double);
    w.cflat = (int*)p;              p += plane * sizeof(int);
    w.cpx = (int*)p;                p += plane * sizeof(int);
    w.cpy = (int*)p;                p += plane * sizeof(int);
    w.cscore = (float*)p;           p += plane * sizeof(int);
    w.rank = (int*)p;               p += plane * sizeof(int);
    w.spx = (int*)p;                p += plane * sizeof(int);
    w.spy = (int*)p;                p += plane * sizeof(int);
    w.sclip = (int*)p;              p += plane * sizeof(int);
    w.mat = (unsigned long long*)p;
    return w;
}

// (1) candidates in flat order; pixel and ratio from slide_project, as slide_detect_kernel takes them
__global__ __launch_bounds__(1024) void samples_compact_kernel(const float* dec, int T, int K, int stride, int padLR,
                                                               int padTB, int clipV, float thr, int x0, int y0, int x1,
                                                               int y1, SamplesWs ws) {
    __shared__ CompactLds<16> cs;
    __shared__ int above_s;
    const int tid = threadIdx.x;
    const int plane = T * K;
    if (tid == 0) { cs.base = 0; above_s = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < plane; c0 += 1024) {
        int q = c0 + tid;
        bool above = false, keep = false;
        int px = 0, py = 0;
        double rt = 0.0;
        float sc = 0.f;
        if (q < plane) {
            sc = dec[q];
            above = sc > thr;
            slide_project(dec, plane, q, K, stride, padLR, padTB, clipV, px, py, rt);
            keep = above && px >= x0 && px < x1 && py >= y0 && py < y1;
        }
        block_count(above, &above_s);
        const int off = block_compact(keep, cs, 16);
        if (keep) {
            ws.cflat[off] = q;
            ws.cpx[off] = px;
            ws.cpy[off] = py;
            ws.cscore[off] = sc;
            ws.cratio[off] = rt;
        }
    }
    if (tid == 0) { ws.hdr[0] = cs.base; ws.hdr[1] = above_s; }
}

// (2) rank by counting: candidates ahead of i have a higher score, or an equal score and a lower flat index (the
// candidates are in flat order, so a lower candidate index).  Scatters pixel and clip into rank order.
__global__ __launch_bounds__(256) void samples_rank_kernel(SamplesWs ws, int K) {
    __shared__ float ssc[256];
    const int n = ws.hdr[0], tid = threadIdx.x;
    if ((int)blockIdx.x * 256 >= n) return;
    const int i = blockIdx.x * 256 + tid;
    const float si = i < n ? ws.cscore[i] : 0.f;
    int r = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        ssc[tid] = j0 + tid < n ? ws.cscore[j0 + tid] : 0.f;
        __syncthreads();
        const int m = min(256, n - j0);
        for (int j = 0; j < m; ++j) {
            float sj = ssc[j];
            r += (sj > si || (sj == si && j0 + j < i)) ? 1 : 0;
        }
    }
    if (i < n) {
        ws.rank[i] = r;
        ws.spx[r] = ws.cpx[i];
        ws.spy[r] = ws.cpy[i];
        ws.sclip[r] = ws.cflat[i] / K;
    }
}

// (3) one wave per 64 x 64 block (row chunk cr, word w <= cr) of the suppression matrix, in rank order
__global__ __launch_bounds__(256) void samples_matrix_kernel(SamplesWs ws, int radius) {
    const int n = ws.hdr[0], lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int C = (n + 63) / 64;
    const long r2 = (long)radius * radius;
    for (long p = (long)blockIdx.x * 4 + wv; p < (long)C * C; p += (long)gridDim.x * 4) {
        const int cr = (int)(p / C), w = (int)(p - (long)cr * C);
        if (w > cr) continue;
        const int r = cr * 64 + lane, c = w * 64 + lane;
        int rx = 0, ry = 0, rc = -1, cx = 0, cy = 0, cc = -1;
        if (r < n) { rx = ws.spx[r]; ry = ws.spy[r]; rc = ws.sclip[r]; }
        if (c < n) { cx = ws.spx[c]; cy = ws.spy[c]; cc = ws.sclip[c]; }
        unsigned long long word = 0;
        for (int j = 0; j < 64; ++j) {
            const int jx = __shfl(cx, j, 64), jy = __shfl(cy, j, 64), jc = __shfl(cc, j, 64);
            const long dx = (long)rx - jx, dy = (long)ry - jy;
            bool near = dx >= -radius && dx <= radius && dy >= -radius && dy <= radius && dx * dx + dy * dy <= r2;
            if (near && w * 64 + j < r && r < n && jc != rc) word |= 1ull << j;   // (a column < r < n is a candidate)
        }
        ws.mat[((long)cr * C + w) * 64 + lane] = word;
    }
}

// (4) resolve the matrix greedily in rank order (radius >= 0), then emit the kept samples in flat order with the
// histogram and the counters.
__global__ __launch_bounds__(1024) void samples_emit_kernel(SamplesWs ws, int radius, double lo, double scale,
                                                            int nbins, int* xy, double* ratio, float* score,
                                                            int* index, int* count, unsigned long long* hist,
                                                            unsigned long long* counters) {
    __shared__ unsigned long long keptw[SS_CAP / 64];
    __shared__ unsigned long long supw[16];
    __shared__ unsigned int lhist[SS_MAXBINS];
    __shared__ CompactLds<16> cs;
    __shared__ int binned_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = ws.hdr[0];
    const int C = (n + 63) / 64;
    for (int b = tid; b < nbins; b += 1024) lhist[b] = 0;
    if (tid == 0) { cs.base = 0; binned_s = 0; }
    __syncthreads();
    if (radius >= 0) {
        for (int c = 0; c < C; ++c) {
            bool f = false;
            for (int w = wv; w < c; w += 16) f = f || (ws.mat[((long)c * C + w) * 64 + lane] & keptw[w]) != 0ull;
            unsigned long long s = __ballot(f);
            if (lane == 0) supw[wv] = s;
            __syncthreads();
            if (wv == 0) {
                s = 0;
                for (int w = 0; w < 16; ++w) s |= supw[w];
                const unsigned long long d = ws.mat[((long)c * C + c) * 64 + lane];
                unsigned long long kw = 0;
                const int rows = min(64, n - c * 64);
                for (int i = 0; i < rows; ++i) {
                    unsigned long long di = __shfl(d, i, 64);
                    if (!((s >> i) & 1ull) && !(di & kw)) kw |= 1ull << i;
                }
                if (lane == 0) keptw[c] = kw;
            }
            __syncthreads();
        }
    }
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + tid;
        bool keep = false, bin = false;
        double rt = 0.0;
        if (i < n) {
            keep = true;
            if (radius >= 0) {
                int r = ws.rank[i];
                keep = (keptw[r >> 6] >> (r & 63)) & 1ull;
            }
            if (keep) {
                rt = ws.cratio[i];
                double v = floor((rt - lo) * scale);
                bin = isfinite(rt) && v >= 0.0 && v < (double)nbins;
                if (bin) atomicAdd(&lhist[(int)v], 1u);
            }
        }
        block_count(bin, &binned_s);
        const int off = block_compact(keep, cs, 16);
        if (keep) {
            xy[2 * off] = ws.cpx[i];
            xy[2 * off + 1] = ws.cpy[i];
            ratio[off] = rt;
            score[off] = ws.cscore[i];
            index[off] = ws.cflat[i];
        }
    }
    for (int b = tid; b < nbins; b += 1024)
        if (lhist[b]) atomicAdd(&hist[b], (unsigned long long)lhist[b]);
    if (tid == 0) {
        *count = cs.base;
        atomicAdd(&counters[0], (unsigned long long)ws.hdr[1]);
        atomicAdd(&counters[1], (unsigned long long)n);
        atomicAdd(&counters[2], (unsigned long long)cs.base);
        atomicAdd(&counters[3], (unsigned long long)binned_s);
        atomicAdd(&counters[4], (unsigned long long)(cs.base - binned_s));
    }
}

}  // namespace

extern "C" size_t scd_slide_samples_workspace(int T, int K) {
    if (T < 1 || K < 1 || (long)T * K > SS_CAP) return 0;
    return samples_ws_bytes((long)T * K);
}

extern "C" int scd_slide_samples(const float* decoded, int T, int K, int stride, int padLR, int padTB, int clipV,
                                 float thr, int x0, int y0, int x1, int y1, int radius, double lo, double scale,
                                 int nbins, int* xy, double* ratio, float* score, int* index, int* count,
                                 int64_t* hist, int64_t* counters, void* workspace, void* stream) {
    if (T < 1 || K < 1 || stride < 1 || clipV < 1 || (long)T * K > SS_CAP || x1 <= x0 || y1 <= y0 || radius < -1 ||
        radius > SCD_SLIDE_RADIUS_MAX || nbins < 1 || nbins > SS_MAXBINS || !(scale == scale) || !(lo == lo))
        return SCD_ERR_ARG;
    if (!decoded || !xy || !ratio || !score || !index || !count || !hist || !counters || !workspace)
        return SCD_ERR_ARG;
    const int plane = T * K;
    SamplesWs ws = samples_ws(workspace, plane);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(samples_compact_kernel, dim3(1), dim3(1024), 0, st, decoded, T, K, stride, padLR, padTB, clipV,
                       thr, x0, y0, x1, y1, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (radius >= 0) {
        // grids cover the slot count; workgroups past the device-side candidate count leave at once
        hipLaunchKernelGGL(samples_rank_kernel, dim3(cdiv(plane, 256)), dim3(256), 0, st, ws, K);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        const long chunks = cdiv(plane, 64);
        hipLaunchKernelGGL(samples_matrix_kernel, dim3((unsigned)min(2048L, (chunks * chunks + 3) / 4)), dim3(256), 0,
                           st, ws, radius);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(samples_emit_kernel, dim3(1), dim3(1024), 0, st, ws, radius, lo, scale, nbins, xy, ratio, score,
                       index, count, (unsigned long long*)hist, (unsigned long long*)counters);
    SCD_RETURN_LAUNCH();
}
