// The environment switches of conv_gemm.hip, which holds every implicit-GEMM kernel family and its launcher.
#pragma once
#include <stdlib.h>

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
