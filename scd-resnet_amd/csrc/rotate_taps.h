// The pixel arithmetic of datasets/argumentations.py:148-159 (rotate with MirrorPadding, Bilinear) shared by the slide
// rotation of preprocess.hip and the per-tile rotation of augment.hip: torch 'reflect' indexing and torchvision's
// bilinear sample of four taps.  Contraction is off from here to the end of the including file (both includers set it
// themselves as well): the operation order below is the contract (at a whole source coordinate the weights are 0 and
// 1 and the sample is the tap itself, bit for bit).
#pragma once
#include "block_ops.h"

#pragma clang fp contract(off)

// the source coordinate (sx, sy) in fp64 -> its cell (x0, y0) and the fp32 weights of the cell's far taps
__device__ __forceinline__ void rot_cell(double sx, double sy, int& x0, int& y0, float& wx, float& wy) {
    const double fx = floor(sx), fy = floor(sy);
    wx = (float)(sx - fx);
    wy = (float)(sy - fy);
    x0 = (int)fx;
    y0 = (int)fy;
}

// two weights and three lerps in fp32
__device__ __forceinline__ float rot_lerp(float v00, float v01, float v10, float v11, float wx, float wy) {
    const float top = v00 * (1.0f - wx) + v01 * wx;
    const float bot = v10 * (1.0f - wx) + v11 * wx;
    return top * (1.0f - wy) + bot * wy;
}
