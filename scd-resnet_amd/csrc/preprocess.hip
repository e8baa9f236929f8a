// Building a `.d` archive on the GPU: the rotated 512 x 512 clips of preprocess.py / datasets/preprocessor/
// scdManual.py:133-186 (reflect-pad the grayscale slide by the margins, rotate about the centre with
// datasets/argumentations.py:148-159 -- a second reflect pad to the diagonal, torchvision's tensor rotate, the
// centre crop -- then cut x-major into tile x tile clips), for all the repeats of one slide at once.
//
// scd_slide_rotate_clips: two launches.  (1) the grayscale plane fp32((0.30 R + 0.59 G) + 0.11 B) (fp64 sum,
// scdManual.py:46-56 followed by rotate's .float()) of the raw slide into the workspace, once, shared by every
// rotation; (2) one thread per four output pixels of a row, grid (row blocks of a tile, clips, rotations): the
// source coordinate in fp64, four taps gathered from the plane through the two nested reflections (no padded or
// rotated slide is ever materialised; the plane of a 2048 x 3072 slide is 25 MB, so the taps are served from the
// L2 / Infinity Cache, and neighbouring lanes read neighbouring plane pixels at the +-15 degrees the preprocessor
// draws), the interpolation in fp32, one float4 store.
#include "rotate_taps.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_ROWS = 8;          // tile rows per workgroup
constexpr int RC_MAXROT = 16;

struct RotGeom {
    const float* grey;      // (H, W) fp32
    int H, W;
    int l, t;               // margins (left, top)
    int Wp, Hp;             // margin-padded frame
    int lp, tp;             // rotate()'s diagonal padding
    int Wq, Hq;             // rotated frame
    int tile, ny;
    double cosA[RC_MAXROT], sinA[RC_MAXROT];
};

__global__ __launch_bounds__(RC_THREADS) void slide_grey_kernel(const uint8_t* rgb, long n, int C, float* grey) {
    for (long i = (long)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * RC_THREADS) {
        const uint8_t* p = rgb + i * C;
        double v = 0.30 * (double)p[0] + 0.59 * (double)p[1];
        v = v + 0.11 * (double)p[2];
        grey[i] = (float)v;
    }
}

// rotated-frame tap -> raw column / row, or -1 when the tap is outside the frame (grid_sample's zeros padding)
__device__ __forceinline__ int tap_index(int tap, int nq, int pad2, int np, int pad1, int n) {
    if (tap < 0 || tap >= nq) return -1;
    return reflect_idx(reflect_idx(tap - pad2, np) - pad1, n);
}

__device__ __forceinline__ float tap_value(const RotGeom& g, int row, int col) {
    return (row < 0 || col < 0) ? 0.0f : g.grey[(long)row * g.W + col];
}

__global__ __launch_bounds__(RC_THREADS) void slide_rotate_kernel(RotGeom g, float* out) {
    const int clip = blockIdx.y, r = blockIdx.z;
    const int cx = clip / g.ny, cy = clip - (clip / g.ny) * g.ny;      // x-major (scdManual.py:182-183)
    const double ca = g.cosA[r], sa = g.sinA[r];
    const double mx = 0.5 * (double)(g.Wq - 1), my = 0.5 * (double)(g.Hq - 1);
    const int quads = g.tile >> 2;
    const int row0 = blockIdx.x * RC_ROWS;
    const int rows = min(RC_ROWS, g.tile - row0);
    float* dst = out + ((long)r * gridDim.y + clip) * g.tile * g.tile;
    for (int it = threadIdx.x; it < rows * quads; it += RC_THREADS) {
        const int i = row0 + it / quads, j0 = (it - (it / quads) * quads) * 4;
        const double yc = (double)(cy * g.tile + i + g.tp) - my;
        float res[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double xc = (double)(cx * g.tile + j0 + k + g.lp) - mx;
            const double sx = (ca * xc - sa * yc) + mx;
            const double sy = (sa * xc + ca * yc) + my;
            int x0, y0;
            float wx, wy;
            rot_cell(sx, sy, x0, y0, wx, wy);
            const int c0 = tap_index(x0, g.Wq, g.lp, g.Wp, g.l, g.W), c1 = tap_index(x0 + 1, g.Wq, g.lp, g.Wp, g.l, g.W);
            const int r0 = tap_index(y0, g.Hq, g.tp, g.Hp, g.t, g.H), r1 = tap_index(y0 + 1, g.Hq, g.tp, g.Hp, g.t, g.H);
            const float v00 = tap_value(g, r0, c0), v01 = tap_value(g, r0, c1);
            const float v10 = tap_value(g, r1, c0), v11 = tap_value(g, r1, c1);
            res[k] = rot_lerp(v00, v01, v10, v11, wx, wy);
        }
        *reinterpret_cast<float4*>(dst + (long)i * g.tile + j0) = make_float4(res[0], res[1], res[2], res[3]);
    }
}

}  // namespace

extern "C" size_t scd_slide_rotate_workspace(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return (size_t)H * (size_t)W * sizeof(float);
}

extern "C" int scd_slide_rotate_clips(const uint8_t* rgb, int H, int W, int C, int left, int top, int right,
                                      int bottom, int tile, const double* angles, int R, float* out,
                                      void* workspace, void* stream) {
    if (H < 2 || W < 2 || C < 3 || tile < 4 || (tile & 3) || R < 1 || R > RC_MAXROT || !angles) return SCD_ERR_ARG;
    if (left < 0 || top < 0 || right < 0 || bottom < 0 || left >= W || right >= W || top >= H || bottom >= H)
        return SCD_ERR_ARG;
    if ((long)H * W >= (1L << 31)) return SCD_ERR_ARG;
    const int Wp = W + left + right, Hp = H + top + bottom;
    if (Wp % tile || Hp % tile) return SCD_ERR_ARG;
    const double radius = sqrt((double)Wp * Wp + (double)Hp * Hp) / 2.0;      // argumentations.py:153-155
    const long lp = (long)ceil(radius - 0.5 * Wp), tp = (long)ceil(radius - 0.5 * Hp);
    if (lp >= Wp || tp >= Hp) return SCD_ERR_ARG;                              // 'reflect' needs pad < size
    const int nx = Wp / tile, ny = Hp / tile;
    if ((long)R * nx * ny * tile * tile >= (1L << 31) || (long)nx * ny > 65535) return SCD_ERR_ARG;
    RotGeom g;
    g.grey = (const float*)workspace;
    g.H = H; g.W = W; g.l = left; g.t = top; g.Wp = Wp; g.Hp = Hp;
    g.lp = (int)lp; g.tp = (int)tp; g.Wq = Wp + 2 * (int)lp; g.Hq = Hp + 2 * (int)tp;
    g.tile = tile; g.ny = ny;
    for (int r = 0; r < RC_MAXROT; ++r) {
        const double a = (r < R ? angles[r] : 0.0) * M_PI / 180.0;
        g.cosA[r] = cos(a);
        g.sinA[r] = sin(a);
    }
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)H * W;
    const long want = (n + RC_THREADS - 1) / RC_THREADS;
    const int gblocks = (int)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(slide_grey_kernel, dim3(gblocks), dim3(RC_THREADS), 0, st, rgb, n, C, (float*)workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(slide_rotate_kernel, dim3((tile + RC_ROWS - 1) / RC_ROWS, nx * ny, R), dim3(RC_THREADS), 0, st,
                       g, out);
    SCD_RETURN_LAUNCH();
}
