// What the GEMM kernels share: the environment switches of conv_gemm.hip (which holds every implicit-GEMM kernel
// family and its launcher), and the addressing and layout rules that conv_gemm.hip, stem.hip, layers.hip and bn.hip
// must agree on -- each stated once here.  A kernel whose generated code changed when it took a helper keeps its own
// copy, with a comment that names the helper.
#pragma once
#include <stdlib.h>

#include "scd_common.h"

// The environment switches of the native library: these five and no other (tests/test_host_cpu.py); every other
// choice is a constant at its use, with its measurement.
// SCD_GEMM_STREAM1X1 (read per call: tests compare the kernels bit for bit): 0 keeps conv1x1_stream_kernel's shapes on
// the tiled kernels, 2 (tests) makes every GEMM the stream kernel does not take fail with SCD_ERR_ARG
static inline int stream1x1_mode() { const char* e = getenv("SCD_GEMM_STREAM1X1"); return e ? atoi(e) : 1; }
// SCD_GEMM_HALO64=0: conv_gemm_l1p_kernel's shapes on the register-staged kernel.  Read per launch (not cached):
// tests switch it to compare the two bit for bit
static inline int halo64_mode() { const char* e = getenv("SCD_GEMM_HALO64"); return e ? atoi(e) : 1; }
// SCD_HEADS_SERP=0: heads384 without the reversed K-stage order on every other round (GemmParams::kserp).  Read per
// call (tests switch it to compare the variants)
static inline int heads_serp_mode() { const char* e = getenv("SCD_HEADS_SERP"); return e ? atoi(e) : 1; }
// SCD_GEMM_PP=0 (read once; tools/dgrad_bench.py): the ping-pong kernel's shapes on the ring / tiled kernels
static inline int pp_mode() { static const int mode = [] { const char* e = getenv("SCD_GEMM_PP"); return e ? atoi(e) : 1; }(); return mode; }
// SCD_GEMM_RING=0/1 (read once; tools/dgrad_bench.py): forces the LDS-DMA ring kernel off / on for the wide bf16 shapes
static inline int ring_mode() { static const int mode = [] { const char* e = getenv("SCD_GEMM_RING"); return e ? atoi(e) : -1; }(); return mode; }

// ---- device rules shared between files (helpers of one file only stay in that file)

// Raw buffer descriptor over `bytes` bytes at p: word 3 = 0x00020000 (raw 32-bit data, no swizzle), so an offset past
// num_records reads zeros and moves nothing -- the kernels mask loads with out-of-range offsets, not branches
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, bytes, 0x00020000);
}

// LDS image of 128-B rows: 16-B chunk c of row r at chunk c ^ (r & 7) (ds_read_b128 fragment reads of 16 consecutive
// rows and ds_write_b128 stores of one row's 8 chunks are then bank-conflict free)
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// LDS image of a [pixel][channel] stage for transposed (ds_read_b64_tr_b16) fragment reads: a row
// stride of 8 dwords mod 64 banks (288 B for <= 256-B rows, 544 B for 512-B rows) puts rows r..r+3 on
// disjoint 8-bank slots, and the column offset of rows with bit 3 set is XORed with 128 B, so rows
// {0-3, 8-11} read by one 32-lane half cover all 64 banks: the transposed reads are conflict free.
__host__ __device__ constexpr int wrow_stride(int rowbytes) { return rowbytes <= 256 ? 288 : rowbytes + 32; }
__device__ __forceinline__ int wswz(int row, int byte, int stride) {
    return row * stride + (byte ^ (((row >> 3) & 1) << 7));
}

// One K-major 8-element MFMA fragment out of an M-major LDS image: two ds_read_b64_tr_b16 (rows r .. r+3 at lo, r+4 ..
// r+7 at hi of the lane's 16-lane group), packed
__device__ __forceinline__ h16x8 tr16_frag(const char* lo_addr, const char* hi_addr) {
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo_addr);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi_addr);
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(h16x8, v);
}

// sum over the 16 lanes of a DPP row (every lane gets it): quad butterflies, then the half-row and row mirrors
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// BN statistics buffer (ops.new_stats / ops.bn_stats size it): fp64 [SCD_STAT_REPLICAS][2][C], stat 0 = sum, 1 = sum of
// squares (backward: sum dz, sum dz * xhat).  A workgroup adds to the replica of its block index (in the caller's
// integer type: the signed and the unsigned remainder are different instructions)
template <typename I>
__device__ __forceinline__ I stat_replica(I block) { return block % SCD_STAT_REPLICAS; }
template <typename I>
__device__ __forceinline__ double* stat_slot(double* stats, I rep, int stat, int C, int c) {
    return stats + ((long)rep * 2 + stat) * C + c;
}

// The end of a 256-thread kernel whose thread t holds the sums s1 / s2 (stat 0 / 1) of the E channels of chunk
// t % cpp (256 % cpp == 0, C = cpp * E): through red (LDS, [2][256][E + 1] floats, free by now) to one fp64 sum per
// channel, threads in ascending order, added to the workgroup's replica
template <int E>
__device__ __forceinline__ void channel_sums_to_slots(const float* s1, const float* s2, float* red, int C, int cpp,
                                                      double* stats) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < E; ++e) { red[tid * (E + 1) + e] = s1[e]; red[(256 + tid) * (E + 1) + e] = s2[e]; }
    __syncthreads();
    for (int k = tid; k < 2 * C; k += 256) {
        const int stat = k / C, c = k - (k / C) * C;
        const int cc = c / E, e = c - (c / E) * E;
        double a = 0.0;
        for (int t = cc; t < 256; t += cpp) a += red[(stat * 256 + t) * (E + 1) + e];
        atomic_add_f64(stat_slot(stats, stat_replica(blockIdx.x), stat, C, c), a);
    }
}
