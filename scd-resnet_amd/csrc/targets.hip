// CenterNet training targets rendered on the GPU: the reference renders them per sample in
// Python (datasets/scds/scdx16p100.py:514-531 object loop, :575-591 drawGaussian, datasets/utility.py:11-16
// gaussianMargin2D, evaluations/intersection.py:46-63 centerThresholdRadius).  One workgroup per tile:
// phase 1 decodes the tile's objects (radius, clipped window, sigma, mask, flat index, regression row) into
// LDS (every workgroup of the tile repeats it; workgroup y == 0 also writes mask / index / regression rows),
// phase 2 walks the workgroup's share of the heatmap pixels and applies the objects IN ORDER per pixel, h = min(f32(g + h), 1)
// with g = exp(-(dx^2 + dy^2) / (2 sigma sigma)) in double -- the reference's float64 Gaussian added to the
// float32 map, rounded back, clipped after every splat -- so overlapping objects clip exactly as there.
// Grid: B tiles x gridDim.y pixel slices (enough workgroups to fill the chip at B = 32).
// scd_render_corner_targets (below) renders the two corner maps of CornerNetLoss with the centre map from the same
// device functions.
#include <math.h>

#include <algorithm>

#include "block_ops.h"

// numpy evaluates every product and sum separately: no fused multiply-adds in this file
#pragma clang fp contract(off)

namespace {

constexpr int MAXOBJ = 64;

struct ObjBox {
    int x, y, l, t, r, b, inside;
    double den;       // 2 * sigma * sigma
};

// centerThresholdRadius (intersection.py:46-63) in the reference's operation order, float64
__device__ double center_radius(double width, double height, double thr) {
    const double a1 = 1, b1 = height + width, c1 = width * height * (1 - thr) / (1 + thr);
    const double r1 = (b1 + sqrt(b1 * b1 - 4 * a1 * c1)) / 2;
    const double a2 = 4, b2 = 2 * (height + width), c2 = (1 - thr) * width * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 4 * a2 * c2)) / 2;
    const double a3 = 4 * thr, b3 = -2 * thr * (height + width), c3 = (thr - 1) * width * height;
    const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
    return fmin(fmin(r1, r2), r3);
}

// The splat of one object, from its row: half window `roi` = ceil(2 radius) and the Gaussian's denominator 2 sigma^2,
// sigma = radius / 3.  The corner maps splat the centre's Gaussian, so this is evaluated once per object.
__device__ __forceinline__ void splat_shape(const float* o, float thr, int& roi, double& den) {
    const float major2 = o[4] * o[4] + o[5] * o[5];    // float32, as the dataset computes it
    const double radius = center_radius(2.0 * sqrt((double)major2), 2.0 * (double)o[6], (double)thr);
    roi = (int)ceil(radius * 2);
    const double sigma = radius / 3;
    den = 2 * sigma * sigma;
}

// the window of a splat at cell (x, y) inside the map, clipped at the map's border
__device__ __forceinline__ void splat_window(ObjBox& bx, int x, int y, int roi, double den, int H) {
    bx.x = x; bx.y = y;
    bx.l = min(roi, x); bx.r = min(roi, H - x - 1);
    bx.t = min(roi, y); bx.b = min(roi, H - y - 1);
    bx.den = den;
}

// the centre's cell of slot k (int(loc[0]), int(loc[1]): truncation) and whether it lies on the map; slots past the
// count are outside
__device__ __forceinline__ int center_cell(const float* o, int k, int cnt, int H, int& x, int& y) {
    x = (int)o[0]; y = (int)o[1];
    return (k < cnt && x >= 0 && x < H && y >= 0 && y < H) ? 1 : 0;
}

// mask / index / regression rows of slot k of tile n (slots past the count stay zero)
__device__ __forceinline__ void write_rows(const float* o, int n, int k, int K, int cnt, int H, int inside,
                                           uint8_t* __restrict__ mask, float* __restrict__ regr,
                                           int64_t* __restrict__ inds) {
    mask[(size_t)n * K + k] = (uint8_t)inside;
    inds[(size_t)n * K + k] = inside ? (int64_t)floorf(o[1]) * H + (int64_t)floorf(o[0]) : 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) regr[((size_t)n * K + k) * 6 + j] = k < cnt ? o[2 + j] : 0.f;
}

// pixel (px, py) of a map: the first cnt boxes applied in slot order
__device__ __forceinline__ float splat_pixel(const ObjBox* box, int cnt, int px, int py) {
    float h = 0.f;
    for (int k = 0; k < cnt; ++k) {
        const ObjBox& bx = box[k];
        if (!bx.inside) continue;
        const int dx = px - bx.x, dy = py - bx.y;
        if (dx < -bx.l || dx > bx.r || dy < -bx.t || dy > bx.b) continue;
        const double g = exp(-(double)(dx * dx + dy * dy) / bx.den);
        const float s = (float)(g + (double)h);
        h = s > 1.f ? 1.f : s;                                // heatmap[heatmap > 1] = 1 (NaN stays NaN)
    }
    return h;
}

__global__ __launch_bounds__(256) void render_center_kernel(const float* __restrict__ locs, const int* __restrict__ counts,
                                                            int K, int H, float thr, float* __restrict__ heat,
                                                            uint8_t* __restrict__ mask, float* __restrict__ regr,
                                                            int64_t* __restrict__ inds) {
    __shared__ ObjBox box[MAXOBJ];
    const int n = blockIdx.x;
    const int cnt = min(counts[n], K);
    const float* L = locs + (size_t)n * K * 8;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float* o = L + k * 8;
        ObjBox bx;
        int x, y;
        bx.inside = center_cell(o, k, cnt, H, x, y);
        if (bx.inside) {
            int roi;
            double den;
            splat_shape(o, thr, roi, den);
            splat_window(bx, x, y, roi, den, H);
        }
        box[k] = bx;
        if (blockIdx.y == 0) write_rows(o, n, k, K, cnt, H, bx.inside, mask, regr, inds);
    }
    __syncthreads();
    float* hm = heat + (size_t)n * H * H;
    for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < H * H; p += gridDim.y * blockDim.x) {
        const int py = p / H, px = p - (p / H) * H;
        hm[p] = splat_pixel(box, cnt, px, py);
    }
}

// ---- scd_render_corner_targets: the centre map and the two corner maps of CornerNetLoss in one launch ------------
// The corner rule is the project's (trainer/dataset/syntheticCorner.py corner_locs; the reference ships no corner
// encoder): top-left = centre - (d_x, d_y), bottom-right = centre + (d_x, d_y), d_x = round(|majx|), d_y = round(minl)
// (half to even), each coordinate clipped to [0, H - 1] and truncated to its cell, all in float32; the splat is the
// centre's (same radius, sigma and window rule).  Completed where the host rule is undefined: a corner is drawn only
// when the object's centre is on the map and both of the corner's coordinates are finite.
// Phase 1 decodes three boxes per object into LDS (3 x 64 x 40 B), the radius once per object; phase 2 is the centre
// kernel's pixel walk, the three maps either looped over by one thread (gridDim.z == 1) or spread over gridDim.z == 3.

// np.clip(v, 0, hi): NaN stays NaN
__device__ __forceinline__ float clip_coord(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// the two corner cells of an object whose centre is on the map (the rule above), and which of them are drawn
struct CornerCells {
    int x0, y0, x1, y1, in0, in1;
};

__device__ __forceinline__ CornerCells corner_cells(const float* o, int H) {
    const float hi = (float)(H - 1);
    const float dx = rintf(fabsf(o[4])), dy = rintf(o[6]);
    const float x0 = clip_coord(o[0] - dx, hi), y0 = clip_coord(o[1] - dy, hi);
    const float x1 = clip_coord(o[0] + dx, hi), y1 = clip_coord(o[1] + dy, hi);
    CornerCells c;
    // finite after the clip means not NaN, and then inside [0, H - 1]
    c.in0 = x0 == x0 && y0 == y0;
    c.in1 = x1 == x1 && y1 == y1;
    c.x0 = c.in0 ? (int)x0 : 0; c.y0 = c.in0 ? (int)y0 : 0;
    c.x1 = c.in1 ? (int)x1 : 0; c.y1 = c.in1 ? (int)y1 : 0;
    return c;
}

__global__ __launch_bounds__(256) void render_corner_kernel(const float* __restrict__ locs, const int* __restrict__ counts,
                                                            int K, int H, float thr, float* __restrict__ heat,
                                                            float* __restrict__ tl, float* __restrict__ br,
                                                            uint8_t* __restrict__ mask, float* __restrict__ regr,
                                                            int64_t* __restrict__ inds) {
    __shared__ ObjBox box[3][MAXOBJ];
    const int n = blockIdx.x;
    const int cnt = min(counts[n], K);
    const float* L = locs + (size_t)n * K * 8;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float* o = L + k * 8;
        ObjBox ct, c0, c1;
        int x, y;
        ct.inside = center_cell(o, k, cnt, H, x, y);
        c0.inside = c1.inside = 0;
        if (ct.inside) {
            int roi;
            double den;
            splat_shape(o, thr, roi, den);
            splat_window(ct, x, y, roi, den, H);
            const CornerCells cc = corner_cells(o, H);
            if (cc.in0) { c0.inside = 1; splat_window(c0, cc.x0, cc.y0, roi, den, H); }
            if (cc.in1) { c1.inside = 1; splat_window(c1, cc.x1, cc.y1, roi, den, H); }
        }
        box[0][k] = ct; box[1][k] = c0; box[2][k] = c1;
        if (blockIdx.y == 0 && blockIdx.z == 0) write_rows(o, n, k, K, cnt, H, ct.inside, mask, regr, inds);
    }
    __syncthreads();
    for (int m = blockIdx.z; m < 3; m += gridDim.z) {
        float* hm = (m == 0 ? heat : m == 1 ? tl : br) + (size_t)n * H * H;
        for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < H * H; p += gridDim.y * blockDim.x) {
            const int py = p / H, px = p - (p / H) * H;
            hm[p] = splat_pixel(box[m], cnt, px, py);
        }
    }
}

// ---- scd_corner_tag_inds: the cells an embedding loss gathers its tags at ---------------------------------------------
// Per slot the flat cell (y * H + x) of the two corners render_corner_kernel draws, from the same center_cell /
// corner_cells; valid exactly when it draws both (slot below the count, centre on the map, both corners finite), else
// both indices are 0.
__global__ void corner_tag_inds_kernel(const float* __restrict__ locs, const int* __restrict__ counts, int B, int K, int H,
                                       int64_t* __restrict__ tl_inds, int64_t* __restrict__ br_inds,
                                       uint8_t* __restrict__ valid) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * K) return;
    const int n = s / K, k = s - n * K;
    const float* o = locs + (size_t)s * 8;
    int x, y, ok = center_cell(o, k, min(counts[n], K), H, x, y);
    CornerCells cc{0, 0, 0, 0, 0, 0};
    if (ok) {
        cc = corner_cells(o, H);
        ok = cc.in0 && cc.in1;
    }
    tl_inds[s] = ok ? (int64_t)cc.y0 * H + cc.x0 : 0;
    br_inds[s] = ok ? (int64_t)cc.y1 * H + cc.x1 : 0;
    valid[s] = (uint8_t)ok;
}

// ---- scd_pack_locs: the label half of a training batch built from a device-resident archive -------------------------
// What SCD.gpu_batch does per tile on the host (trainer/dataset/scdx16p100.py: flipLocs, rotateLocs, _pack_locs), one
// workgroup per tile: the tile's CSR rows, flipped, with a rotation each row's nine replicas turned in float32 in the
// host's operation order (datasets/preprocessor/scdManual.py _turn / rotateCoordinates) and filtered by the truncated
// centre, compacted in candidate order into the first K slots.

constexpr int PACK_THREADS = 256;

// _turn: (x, y) turned through its length m and direction (x / m, y / m); a zero vector gives NaN.  Every operation
// rounds once, as numpy's float32 does: plain operators written in this file, so the `fp contract(off)` above holds
// for them (the __f*_rn helpers are header functions the pragma does not reach, and __fsqrt_rn is the 1-ulp hardware
// sqrt), and sqrtf / the division, which hipcc rounds correctly by default.
__device__ __forceinline__ void pack_turn(float x, float y, float ca, float sa, float& ox, float& oy, float& m) {
    m = sqrtf(x * x + y * y);
    const float s = y / m, c = x / m;
    ox = m * (c * ca - s * sa);
    oy = m * (s * ca + c * sa);
}

__global__ __launch_bounds__(PACK_THREADS) void pack_locs_kernel(const float* __restrict__ rows,
                                                                 const long* __restrict__ offsets,
                                                                 const int* __restrict__ ids,
                                                                 const uint8_t* __restrict__ flips,
                                                                 const float* __restrict__ cs, int size, int K, int trunc,
                                                                 float* __restrict__ locs, int* __restrict__ counts) {
    __shared__ CompactLds<PACK_THREADS / 64> cl;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long r0 = offsets[ids[b]];
    const long n = offsets[ids[b] + 1] - r0;
    const bool rot = cs != nullptr;
    const long ncand = rot ? 9 * n : n;
    const bool fx = flips && flips[b * 2], fy = flips && flips[b * 2 + 1];
    const float ca = rot ? cs[b * 2] : 1.f, sa = rot ? cs[b * 2 + 1] : 0.f;
    const float edge = (float)(size - 1), far = (float)(2 * size - 1), fsize = (float)size;
    const float shift = (float)(0.5 - (double)(size / 2));
    float* out = locs + (long)b * K * 8;
    if (tid == 0) cl.base = 0;
    __syncthreads();
    for (long c0 = 0; c0 < ncand && cl.base < K; c0 += PACK_THREADS) {
        const long c = c0 + tid;
        bool keep = false;
        float v[8];
        if (c < ncand) {
            const long row = rot ? c / 9 : c;
            const int k = rot ? (int)(c - row * 9) : 0;
            const float4 lo = *(const float4*)(rows + (r0 + row) * 8), hi = *(const float4*)(rows + (r0 + row) * 8 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
            v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            if (fx) { v[0] = edge - v[0]; v[2] = -v[2]; v[4] = -v[4]; }       // flipLocs
            if (fy) { v[1] = edge - v[1]; v[3] = -v[3]; v[5] = -v[5]; }
            keep = true;
            if (rot) {
                const int kx = k / 3, ky = k - kx * 3;                                  // rotateLocs' replica k
                if (kx) { v[0] = kx == 1 ? far - v[0] : -1.f - v[0]; v[2] = -v[2]; v[4] = -v[4]; }
                if (ky) { v[1] = ky == 1 ? -1.f - v[1] : far - v[1]; v[3] = -v[3]; v[5] = -v[5]; }
                const float sx = v[0] + shift, sy = v[1] + shift;   // rotateCoordinates
                if (!(sx == 0.f && sy == 0.f)) {          // a centre on the rotation centre stays where it is
                    float tx, ty, m;
                    pack_turn(sx, sy, ca, sa, tx, ty, m);
                    v[0] = tx - shift;
                    v[1] = ty - shift;
                }
                float ox, oy, len;
                pack_turn(v[2], v[3], ca, sa, ox, oy, len);
                v[2] = len == 0.f ? 0.f : ox;                                           // a zero offset stays zero
                v[3] = len == 0.f ? 0.f : oy;
                pack_turn(v[4], v[5], ca, sa, ox, oy, len);                             // a zero major axis: NaN
                v[4] = ox; v[5] = oy;
                const float cx = truncf(v[0]), cy = truncf(v[1]);                       // NaN compares false: dropped
                keep = cx >= 0.f && cx < fsize && cy >= 0.f && cy < fsize;
            }
        }
        const int off = block_compact(keep, cl, PACK_THREADS / 64);
        if (keep && off < K) {
            if (trunc) { v[0] = truncf(v[0]); v[1] = truncf(v[1]); }
            *(float4*)(out + off * 8) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)(out + off * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
    const int cnt = min(cl.base, K);
    if (tid == 0) counts[b] = cnt;
    for (int i = cnt * 8 + tid; i < K * 8; i += PACK_THREADS) out[i] = 0.f;
}

}  // namespace

extern "C" int scd_pack_locs(const float* rows, const long* offsets, const int* ids, int B, const uint8_t* flips,
                             const float* cs, int size, int K, int trunc, float* locs, int* counts, void* stream) {
    if (!rows || !offsets || !ids || !locs || !counts || B < 1 || size < 1 || K < 1 || K > MAXOBJ) return SCD_ERR_ARG;
    hipLaunchKernelGGL(pack_locs_kernel, dim3(B), dim3(PACK_THREADS), 0, (hipStream_t)stream, rows, offsets, ids, flips,
                       cs, size, K, trunc, locs, counts);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_render_center_targets(const float* locs, const int* counts, int B, int K, int H, float threshold,
                                         float* heat, uint8_t* mask, float* regr, int64_t* inds, void* stream) {
    if (B < 1 || K < 1 || K > MAXOBJ || H < 1 || (long)H * H >= (1L << 31)) return SCD_ERR_ARG;
    const int slices = std::max(1, std::min(64, cdiv((long)H * H, 256)));
    hipLaunchKernelGGL(render_center_kernel, dim3(B, slices), dim3(256), 0, (hipStream_t)stream, locs, counts, K, H, threshold,
                       heat, mask, regr, inds);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_render_corner_targets_split(const float* locs, const int* counts, int B, int K, int H, float threshold,
                                               float* heat, float* tl, float* br, uint8_t* mask, float* regr,
                                               int64_t* inds, int split, void* stream) {
    if (!locs || !counts || !heat || !tl || !br || !mask || !regr || !inds) return SCD_ERR_ARG;
    if (B < 1 || K < 1 || K > MAXOBJ || H < 1 || (long)H * H >= (1L << 31)) return SCD_ERR_ARG;
    if (split != SCD_CORNER_SPLIT_THREAD && split != SCD_CORNER_SPLIT_GRID) return SCD_ERR_ARG;
    const int slices = std::max(1, std::min(64, cdiv((long)H * H, 256)));
    const int maps = split == SCD_CORNER_SPLIT_GRID ? 3 : 1;
    hipLaunchKernelGGL(render_corner_kernel, dim3(B, slices, maps), dim3(256), 0, (hipStream_t)stream, locs, counts, K, H,
                       threshold, heat, tl, br, mask, regr, inds);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_render_corner_targets(const float* locs, const int* counts, int B, int K, int H, float threshold,
                                         float* heat, float* tl, float* br, uint8_t* mask, float* regr, int64_t* inds,
                                         void* stream) {
    return scd_render_corner_targets_split(locs, counts, B, K, H, threshold, heat, tl, br, mask, regr, inds,
                                           SCD_CORNER_SPLIT_DEFAULT, stream);
}

extern "C" int scd_corner_tag_inds(const float* locs, const int* counts, int B, int K, int size, int64_t* tl_inds,
                                   int64_t* br_inds, uint8_t* valid, void* stream) {
    if (!locs || !counts || !tl_inds || !br_inds || !valid) return SCD_ERR_ARG;
    if (B < 1 || K < 1 || K > MAXOBJ || size < 1 || (long)size * size >= (1L << 31) || (long)B * K >= (1L << 28))
        return SCD_ERR_ARG;
    hipLaunchKernelGGL(corner_tag_inds_kernel, dim3(cdiv((long)B * K, 256)), dim3(256), 0, (hipStream_t)stream, locs,
                       counts, B, K, size, tl_inds, br_inds, valid);
    SCD_RETURN_LAUNCH();
}
