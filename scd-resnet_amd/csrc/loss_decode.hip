// CenterNet loss (focal.py:25-53, regression.py:37-44, centerNetOffset.py:182-217) and
// decode (centerNetOffset.py:219-251, utility.py:87-118) on device, with no host syncs:
// normalisers (#pos, #mask) stay in device memory and are consumed by the backward scale.
#define BLOCK_OPS_FP
#include "block_ops.h"

namespace {

__global__ void focal_fwd_kernel(const float* x, const float* gt, long n, float* g, double* acc) {
    float posl = 0.f, negl = 0.f, npos = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        g[i] = focal_logit_term(x[i], gt[i], posl, negl, npos);
    focal_accumulate(posl, negl, npos, acc);
}

// masked L1 on features gathered at inds (NCHW fp32).  g must be zero on entry.
__global__ void l1_gather_kernel(const float* feat, int N, int C, int HW, const int64_t* inds, const uint8_t* mask,
                                 const float* target, int K, int tstride, int toff, float* g, double* acc) {
    float s = 0.f, cnt = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N * K; i += gridDim.x * blockDim.x) {
        const int n = i / K;
        if (!mask[i]) continue;
        cnt += 1.f;
        const long ind = inds[i];
        // (the same loop as centernet_loss_b_kernel's: as a shared function it cost this kernel 2 instructions)
        for (int c = 0; c < C; ++c) {
            const long fi = ((long)n * C + c) * HW + ind;
            const float d = feat[fi] - target[(long)i * tstride + toff + c];
            s += fabsf(d);
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            if (sg != 0.f) atomic_add_f32(g + fi, sg);
        }
    }
    double a = (double)s, b = (double)cnt;
    if (block_sums_d<4>(a, b, blockDim.x / 64)) {
        atomic_add_f64(acc + 0, a);
        atomic_add_f64(acc + 1, b);
    }
}

struct LossFin {
    float l1w[8];
};

// focal term f from its accumulator replicas (focal.py:47-51: no positives -> -negL ; else -(posL+negL)/#pos) and
// the factor its saved gradient is scaled by in backward
__device__ __forceinline__ float focal_finalize(const double* facc, int f, float* factor) {
    double pl = 0, nl = 0, np = 0;
    for (int r = 0; r < SCD_STAT_REPLICAS; ++r) {
        const double* a = facc + ((long)f * SCD_STAT_REPLICAS + r) * FOCAL_ACC;
        pl += a[0]; nl += a[1]; np += a[2];
    }
    const float posl = (float)pl, negl = (float)nl, npos = (float)np;
    *factor = np == 0.0 ? -1.f : -1.f / npos;
    return np == 0.0 ? -negl : -(posl + negl) / npos;
}

// one block of 64 threads: thread 0 forms the loss terms, then the block re-zeroes both accumulators
// (persistent, consumer-cleared buffers: no memset launch before the next step's loss)
__global__ void loss_finalize_kernel(double* facc, int nfocal, double* lacc, int nl1, LossFin w, float* out,
                                     float* factors) {
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int f = 0; f < nfocal; ++f) {
            const float v = focal_finalize(facc, f, factors + f);
            out[1 + f] = v;
            total += v;
        }
        for (int l = 0; l < nl1; ++l) {
            const double s = lacc[2 * l], cnt = lacc[2 * l + 1];
            const float v = w.l1w[l] * ((float)s / ((float)cnt + 1e-4f));
            out[1 + nfocal + l] = v;
            factors[nfocal + l] = w.l1w[l] / ((float)cnt + 1e-4f);
            total += v;
        }
        out[0] = (float)total;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nfocal * SCD_STAT_REPLICAS * FOCAL_ACC; i += blockDim.x) facc[i] = 0.0;
    if (lacc)
        for (int i = threadIdx.x; i < 2 * nl1; i += blockDim.x) lacc[i] = 0.0;
}

__global__ void scale_by_device_kernel(float* g, long n, const float* factors, int idx, const float* go) {
    const float f = factors[idx] * (go ? go[0] : 1.f);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] *= f;
}

// ---------------------------------------------------------------- CenterNetLoss in two launches
// (centerNetOffset.py:182-217): (A) focal loss + gradient on the heatmap and the zero fill of the size / offset
// gradient buffer (both element-wise over the batch); (B) one workgroup: the two masked L1 terms on the gathered
// size / offset values (gradient +-1 added at the gathered pixels: integer-valued, so exact in any order), then the
// finalize of loss_finalize_kernel (focal replicas + L1 sums -> loss, stats, backward factors).
__global__ void centernet_loss_a_kernel(const float* x, const float* gt, long n, float* g, double* acc, float* gz,
                                        long nz) {
    float posl = 0.f, negl = 0.f, npos = 0.f;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride)
        g[i] = focal_logit_term(x[i], gt[i], posl, negl, npos);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nz; i += stride) gz[i] = 0.f;
    focal_accumulate(posl, negl, npos, acc);
}

static_assert(SCD_STAT_REPLICAS == 64, "centernet_loss_b_kernel sums the focal replicas with one wave");

struct L1Term {
    const float* feat;
    float* g;
    int C, toff;
};

__global__ __launch_bounds__(1024) void centernet_loss_b_kernel(int N, int HW, const int64_t* inds, const uint8_t* mask,
                                                               const float* target, int K, int tstride, L1Term t0,
                                                               L1Term t1, double* facc, LossFin w, float* out,
                                                               float* factors) {
    float s[2] = {0.f, 0.f}, cnt = 0.f;
    for (int i = threadIdx.x; i < N * K; i += blockDim.x) {
        if (!mask[i]) continue;
        cnt += 1.f;
        const int n = i / K;
        const long ind = inds[i];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const L1Term& t = l ? t1 : t0;
            for (int c = 0; c < t.C; ++c) {
                const long fi = ((long)n * t.C + c) * HW + ind;
                const float d = t.feat[fi] - target[(long)i * tstride + t.toff + c];
                s[l] += fabsf(d);
                const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                if (sg != 0.f) atomic_add_f32(t.g + fi, sg);
            }
        }
    }
    // (block_sums_d and focal_finalize written out: the replica sums share the barrier, and through the helpers the
    // kernel took 26 more instructions)
    __shared__ double red[3][16], frd[3];
    const double a = wave_sum_d((double)s[0]), b = wave_sum_d((double)s[1]), c = wave_sum_d((double)cnt);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[0][wv] = a; red[1][wv] = b; red[2][wv] = c; }
    if (wv == 0) {
        // the focal replicas: one lane each (SCD_STAT_REPLICAS == 64), summed across the wave
        const double* q = facc + (long)lane * FOCAL_ACC;
        const double pl = wave_sum_d(q[0]), nl = wave_sum_d(q[1]), np = wave_sum_d(q[2]);
        if (lane == 0) { frd[0] = pl; frd[1] = nl; frd[2] = np; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ls[2] = {0.0, 0.0}, lc = 0.0;
        for (int k = 0; k < (int)(blockDim.x / 64); ++k) { ls[0] += red[0][k]; ls[1] += red[1][k]; lc += red[2][k]; }
        const double pl = frd[0], nl = frd[1], np = frd[2];
        // focal.py:47-51: no positives -> -negL ; else -(posL+negL)/#pos; regression.py:37-44: sum|d| / (#mask + 1e-4)
        const float posl = (float)pl, negl = (float)nl, npos = (float)np;
        const float v = np == 0.0 ? -negl : -(posl + negl) / npos;
        out[1] = v;
        factors[0] = np == 0.0 ? -1.f : -1.f / npos;
        double total = v;
        for (int l = 0; l < 2; ++l) {
            const float vl = w.l1w[l] * ((float)ls[l] / ((float)lc + 1e-4f));
            out[2 + l] = vl;
            factors[1 + l] = w.l1w[l] / ((float)lc + 1e-4f);
            total += vl;
        }
        out[0] = (float)total;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SCD_STAT_REPLICAS * FOCAL_ACC; i += blockDim.x) facc[i] = 0.0;
}

// backward: g_heat *= factors[0] * go (dense); the size / offset gradients are zero except at the gathered pixels,
// so only those are scaled (factors[1], factors[2]), each pixel once (its first slot in the image)
__global__ void centernet_loss_scale_kernel(float* gh, long nh, int N, int HW, const int64_t* inds, int K, float* g0,
                                            int C0, float* g1, int C1, const float* factors, const float* go) {
    const float gs = go ? go[0] : 1.f;
    const float f0 = factors[0] * gs;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long i = t0; i < nh; i += stride) gh[i] *= f0;
    const float f1 = factors[1] * gs, f2 = factors[2] * gs;
    for (long s = t0; s < (long)N * K; s += stride) {
        const int n = (int)(s / K), k = (int)(s - (long)n * K);
        const int64_t ind = inds[s];
        if (ind < 0 || ind >= HW) continue;
        bool first = true;
        for (int k2 = 0; k2 < k; ++k2) first &= inds[(long)n * K + k2] != ind;
        if (!first) continue;
        for (int c = 0; c < C0; ++c) g0[((long)n * C0 + c) * HW + ind] *= f1;
        for (int c = 0; c < C1; ++c) g1[((long)n * C1 + c) * HW + ind] *= f2;
    }
}

// ---------------------------------------------------------------- decode
// (the map t[n][i] = sigmoid(x) kept where it equals its 3x3 max, else 0, is nms_kernel<NmsSigmoid>)
// The K largest of n candidates, sorted, for one workgroup: cand(i, bits) says whether candidate i takes part and
// gives its score's bit pattern (non-negative floats order like their bit patterns).  Radix-select the K-th largest
// (four 8-bit passes), collect, then bitonic sort by (score desc, index asc).  At least K candidates must take part,
// K <= 1024; on return keys[0..K) hold (bits << 32) | (0xFFFFFFFF - index), every thread past a barrier.
template <typename Cand>
__device__ __forceinline__ void select_sorted_keys(Cand cand, int n, int K, unsigned long long* keys) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_krem, s_count, s_eqtaken;
    const int tid = threadIdx.x;
    unsigned prefix = 0, pmask = 0, krem = (unsigned)K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += blockDim.x) {
            unsigned b;
            if (cand(i, b) && (b & pmask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0, d = 0;
            for (int b = 255; b >= 0; --b) {
                if (cum + hist[b] >= krem) { d = (unsigned)b; break; }
                cum += hist[b];
            }
            s_prefix = prefix | (d << shift);
            s_krem = krem - cum;
        }
        __syncthreads();
        prefix = s_prefix;
        krem = s_krem;
        pmask |= 255u << shift;
        __syncthreads();
    }
    // prefix = bits of the K-th largest value; krem = how many elements equal to it are needed
    if (tid == 0) { s_count = 0; s_eqtaken = 0; }
    for (int i = tid; i < 1024; i += blockDim.x) keys[i] = 0ull;
    __syncthreads();
    const unsigned thr = prefix;
    for (int i = tid; i < n; i += blockDim.x) {
        unsigned b;
        if (cand(i, b) && b > thr) {
            const unsigned slot = atomicAdd(&s_count, 1u);
            keys[slot] = ((unsigned long long)b << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
        }
    }
    __syncthreads();
    // ties at the threshold: take the lowest indices, in index order (chunks of blockDim); block_compact written out
    // with the barrier at the top (through the helper the decode and the pairing took 21 more instructions)
    for (int base = 0; base < n; base += blockDim.x) {
        __syncthreads();
        const unsigned taken = s_eqtaken;
        if (taken >= krem) break;
        const int i = base + tid;
        unsigned b = 0;
        const bool eq = i < n && cand(i, b) && b == thr;
        // block-wide exclusive prefix count of eq flags
        const unsigned long long bal = __ballot(eq);
        const int lane = tid & 63, wv = tid >> 6;
        __shared__ unsigned wcount[16];
        if (lane == 0) wcount[wv] = __popcll(bal);
        __syncthreads();
        unsigned before = 0;
        for (int k = 0; k < wv; ++k) before += wcount[k];
        before += __popcll(bal & ((1ull << lane) - 1ull));
        if (eq && taken + before < krem) {
            const unsigned slot = (unsigned)K - krem + taken + before;
            keys[slot] = ((unsigned long long)thr << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned tot = 0;
            for (int k = 0; k < (int)(blockDim.x / 64); ++k) tot += wcount[k];
            s_eqtaken = taken + tot;
        }
    }
    __syncthreads();
    // bitonic sort keys[0..P) descending (P = next pow2 >= K, zero keys sort last)
    int P = 1;
    while (P < K) P <<= 1;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P; i += blockDim.x) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = (i & size) == 0;
                    const unsigned long long a = keys[i], b = keys[j];
                    if (desc ? (a < b) : (a > b)) { keys[i] = b; keys[j] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// one 1024-thread block per image: the K largest NMS'd scores (select_sorted_keys over the map's pixels) and the
// gathers at them
__global__ __launch_bounds__(1024) void decode_select_kernel(const float* t, int HW, int W, int K,
                                                             const float* offset, int od_off, const float* regr,
                                                             int od_regr, float* scores, int64_t* inds, int64_t* ys,
                                                             int64_t* xs, float* off_out, float* regr_out) {
    __shared__ unsigned long long keys[1024];
    const int n = blockIdx.x;
    const unsigned* bits = (const unsigned*)(t + (long)n * HW);
    const int tid = threadIdx.x;
    select_sorted_keys([bits](int i, unsigned& b) { b = bits[i]; return true; }, HW, K, keys);
    for (int k = tid; k < K; k += blockDim.x) {
        const unsigned long long key = keys[k];
        const unsigned b = (unsigned)(key >> 32);
        const int idx = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
        const long o = (long)n * K + k;
        scores[o] = __uint_as_float(b);
        inds[o] = idx;
        ys[o] = idx / W;
        xs[o] = idx % W;
        for (int c = 0; c < od_off; ++c) off_out[o * od_off + c] = offset[((long)n * od_off + c) * HW + idx];
        if (regr)
            for (int c = 0; c < od_regr; ++c) regr_out[o * od_regr + c] = regr[((long)n * od_regr + c) * HW + idx];
    }
}

// ---------------------------------------------------------------- CornerNet: corner pairing
// decodeCornerNet's K x K pairing (cornerNetLegacy.py:332-446) for one category, one workgroup per image: the
// candidates (i, j) -- top-left corner i with bottom-right corner j -- are formed on the fly from the K-length arrays
// in LDS, never stored.  score = (s_tl[i] + s_br[j]) / 2; a pair is dropped when |tag_tl[i] - tag_br[j]| > threshold,
// x_br < x_tl or y_br < y_tl.  The D best survivors by (score desc, flat index i*K + j asc) become rows
// [x_tl, y_tl, x_br, y_br, score, s_tl, s_br, 0]; the rest of the D rows have score -1 and zeros.  Scores must be
// non-negative (they are sigmoids); a corner whose index lies outside the map pairs with nothing.
constexpr int PAIR_MAXK = 128;

__global__ __launch_bounds__(1024) void corner_pairs_kernel(const float* s_tl, const int64_t* i_tl, const int64_t* y_tl,
                                                            const int64_t* x_tl, const float* s_br, const int64_t* i_br,
                                                            const int64_t* y_br, const int64_t* x_br, const float* tag_tl,
                                                            const float* tag_br, int K, int HW, float threshold, int D,
                                                            float* det, int* nvalid) {
    __shared__ unsigned long long keys[1024];
    __shared__ float sc[2][PAIR_MAXK], tg[2][PAIR_MAXK];
    __shared__ int cx[2][PAIR_MAXK], cy[2][PAIR_MAXK], ok[2][PAIR_MAXK];
    __shared__ unsigned s_nvalid;
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < 2 * K; k += blockDim.x) {
        const int c = k >= K, kk = k - c * K;
        const long o = (long)n * K + kk;
        const int64_t ind = (c ? i_br : i_tl)[o];
        const bool in = ind >= 0 && ind < HW;
        sc[c][kk] = (c ? s_br : s_tl)[o];
        tg[c][kk] = in ? (c ? tag_br : tag_tl)[(long)n * HW + ind] : 0.f;
        cx[c][kk] = (int)(c ? x_br : x_tl)[o];
        cy[c][kk] = (int)(c ? y_br : y_tl)[o];
        ok[c][kk] = in;
    }
    if (tid == 0) s_nvalid = 0;
    __syncthreads();
    auto cand = [&](int f, unsigned& b) {
        const int i = f / K, j = f - i * K;
        b = __float_as_uint((sc[0][i] + sc[1][j]) * 0.5f);
        return ok[0][i] && ok[1][j] && !(fabsf(tg[0][i] - tg[1][j]) > threshold) && !(cx[1][j] < cx[0][i]) &&
               !(cy[1][j] < cy[0][i]);
    };
    unsigned mine = 0;
    for (int f = tid; f < K * K; f += blockDim.x) {
        unsigned b;
        mine += cand(f, b) ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_nvalid, mine);
    __syncthreads();
    const int nsel = min((int)s_nvalid, D);
    __syncthreads();
    if (nsel > 0) select_sorted_keys(cand, K * K, nsel, keys);
    float* out = det + (long)n * D * 8;
    for (int r = tid; r < D; r += blockDim.x) {
        float row[8] = {0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f};
        if (r < nsel) {
            const unsigned long long key = keys[r];
            const int f = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
            const int i = f / K, j = f - i * K;
            row[0] = (float)cx[0][i]; row[1] = (float)cy[0][i]; row[2] = (float)cx[1][j]; row[3] = (float)cy[1][j];
            row[4] = __uint_as_float((unsigned)(key >> 32)); row[5] = sc[0][i]; row[6] = sc[1][j];
        }
        *(float4*)(out + r * 8) = make_float4(row[0], row[1], row[2], row[3]);
        *(float4*)(out + r * 8 + 4) = make_float4(row[4], row[5], row[6], row[7]);
    }
    if (tid == 0) nvalid[n] = nsel;
}

// ---------------------------------------------------------------- CornerNet: associative-embedding loss
// embeddingLoss (models/losses/embeddings.py) with the pair mask its comment describes (a uint8 mask; with a bool mask
// the reference's `mask + mask` stays bool, `.eq(2)` is false everywhere and push is 0: DESIGN §8f).  Per image b
// with n valid slots, e_tl[k] / e_br[k] the tags at the slots' corner cells, m = (e_tl + e_br) / 2:
//   pull = sum_{k valid} [(e_tl - m)^2 + (e_br - m)^2] / (n + 1e-4)
//   push = sum_{i, j valid} [relu(1 - |m_i - m_j|) - 1 / (n + 1e-4)] / (n (n - 1) + 1e-4)      (diagonal included)
// One workgroup per image; sums in double, written (not added) to the image's two accumulator slots, so the finalize
// sums them in image order and nothing needs zeroing.  The per-slot gradients (torch's conventions: d|x|/dx = 0 at 0,
// relu' = 0 at 0), already times w_pull / w_push, go to gs_tl / gs_br (N, K); the backward scatters them.
constexpr int AE_MAXK = 64;
constexpr int AE_THREADS = 256;

__global__ __launch_bounds__(AE_THREADS) void corner_ae_fwd_kernel(const float* tl_tag, const float* br_tag, int HW,
                                                                   const int64_t* tl_inds, const int64_t* br_inds,
                                                                   const uint8_t* valid, int K, float w_pull,
                                                                   float w_push, double* acc, float* gs_tl,
                                                                   float* gs_br) {
    __shared__ double et[AE_MAXK], eb[AE_MAXK], mm[AE_MAXK];
    __shared__ int vd[AE_MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < K) {
        const long o = (long)b * K + tid;
        const int64_t it = tl_inds[o], ib = br_inds[o];
        const int v = valid[o] && it >= 0 && it < HW && ib >= 0 && ib < HW;
        vd[tid] = v;
        et[tid] = v ? (double)tl_tag[(long)b * HW + it] : 0.0;
        eb[tid] = v ? (double)br_tag[(long)b * HW + ib] : 0.0;
        mm[tid] = (et[tid] + eb[tid]) / 2;
    }
    __syncthreads();
    int n = 0;
    for (int k = 0; k < K; ++k) n += vd[k];
    // the reference's normalisers are float32 whatever the tags' dtype (mask.sum().float() + 1e-4 and its reciprocal)
    const float fn = (float)n;
    const float dpull_f = fn + 1e-4f, dpush_f = (fn - 1.f) * fn + 1e-4f;
    const double dpull = (double)dpull_f, dpush = (double)dpush_f, inv = (double)(1.f / dpull_f);
    double pull = 0.0, push = 0.0;
    if (tid < K && vd[tid]) {
        const double a = et[tid] - mm[tid], c = eb[tid] - mm[tid];
        pull = a * a / dpull + c * c / dpull;
    }
    for (int f = tid; f < K * K; f += blockDim.x) {
        const int i = f / K, j = f - i * K;
        if (!(vd[i] && vd[j])) continue;
        push += (fmax(1.0 - fabs(mm[j] - mm[i]), 0.0) - inv) / dpush;
    }
    if (block_sums_d<AE_THREADS / 64>(pull, push, AE_THREADS / 64)) {
        acc[2 * b] = pull;
        acc[2 * b + 1] = push;
    }
    if (tid < K) {
        double gt = 0.0, gb = 0.0;
        if (vd[tid]) {
            // pull: d/de_tl = 2 (e_tl - m) (1 - 1/2) + 2 (e_br - m) (-1/2) = (e_tl - m) - (e_br - m), over (n + 1e-4)
            const double gp = ((et[tid] - mm[tid]) - (eb[tid] - mm[tid])) / dpull;
            // push: m_i stands in the pairs (i, j) and (j, i); each gives -sign(m_i - m_j) where 1 - |..| > 0
            double cnt = 0.0;
            for (int j = 0; j < K; ++j) {
                if (!vd[j]) continue;
                const double d = mm[tid] - mm[j];
                if (1.0 - fabs(d) > 0.0) cnt += d > 0.0 ? -1.0 : (d < 0.0 ? 1.0 : 0.0);
            }
            const double gm = 2.0 * cnt / dpush * 0.5;          // dm/de = 1/2 on both corners
            gt = (double)w_pull * gp + (double)w_push * gm;
            gb = -(double)w_pull * gp + (double)w_push * gm;
        }
        gs_tl[(long)b * K + tid] = (float)gt;
        gs_br[(long)b * K + tid] = (float)gb;
    }
}

// focal terms (FocalOnlyLossFn's finalize) + the embedding sums in image order -> out = [loss, focal x nfocal, w_pull
// pull, w_push push], the focal backward factors; re-zeroes the focal replicas (consumer-cleared)
__global__ void corner_ae_finalize_kernel(double* facc, int nfocal, const double* acc, int N, float w_pull, float w_push,
                                          float* out, float* factors) {
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int f = 0; f < nfocal; ++f) {
            const float v = focal_finalize(facc, f, factors + f);
            out[1 + f] = v;
            total += v;
        }
        double pull = 0.0, push = 0.0;
        for (int b = 0; b < N; ++b) { pull += acc[2 * b]; push += acc[2 * b + 1]; }
        const float vp = w_pull * (float)pull, vq = w_push * (float)push;
        out[1 + nfocal] = vp;
        out[2 + nfocal] = vq;
        out[0] = (float)(total + vp + vq);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nfocal * SCD_STAT_REPLICAS * FOCAL_ACC; i += blockDim.x) facc[i] = 0.0;
}

// backward: the two tag gradient maps (N, 1, H, W) written whole -- every pixel the sum, in slot order, of the slot
// gradients of the valid slots that name it (two objects may share a corner cell), times the incoming gradient; zero
// elsewhere.  One thread per pixel, so the sum is deterministic and no zero fill or atomic is needed.
__global__ __launch_bounds__(256) void corner_ae_bwd_kernel(const float* gs_tl, const float* gs_br,
                                                            const int64_t* tl_inds, const int64_t* br_inds,
                                                            const uint8_t* valid, int K, int HW, const float* go,
                                                            float* g_tl, float* g_br) {
    __shared__ float gs[2][AE_MAXK];
    __shared__ int ix[2][AE_MAXK];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 2 * K) {
        const int c = tid >= K, k = tid - c * K;
        const long o = (long)b * K + k;
        gs[c][k] = (c ? gs_br : gs_tl)[o];
        const int64_t ind = (c ? br_inds : tl_inds)[o];
        ix[c][k] = (valid[o] && ind >= 0 && ind < HW) ? (int)ind : -1;
    }
    __syncthreads();
    const float s = go ? go[0] : 1.f;
    for (int p = blockIdx.x * blockDim.x + tid; p < HW; p += gridDim.x * blockDim.x) {
        float a = 0.f, c = 0.f;
        for (int k = 0; k < K; ++k) {
            if (ix[0][k] == p) a += gs[0][k];
            if (ix[1][k] == p) c += gs[1][k];
        }
        g_tl[(long)b * HW + p] = a * s;
        g_br[(long)b * HW + p] = c * s;
    }
}

}  // namespace

extern "C" int scd_focal_fwd(const float* logits, const float* gt, long n, float* g, double* acc, void* stream) {
    hipLaunchKernelGGL(focal_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, logits, gt, n, g, acc);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_l1_gather_fwd(const float* feat, int N, int C, int HW, const int64_t* inds, const uint8_t* mask,
                                 const float* target, int K, int tstride, int toff, float* g, double* acc, void* stream) {
    const int blocks = std::max(1, std::min(64, cdiv((long)N * K, 256)));
    hipLaunchKernelGGL(l1_gather_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, feat, N, C, HW, inds, mask,
                       target, K, tstride, toff, g, acc);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_centernet_loss_finalize(double* focal_acc, int nfocal, double* l1_acc, int nl1,
                                           const float* l1_weights, float* out, float* factors, void* stream) {
    if (nl1 > 8) return SCD_ERR_ARG;
    LossFin w;
    for (int i = 0; i < 8; ++i) w.l1w[i] = i < nl1 ? l1_weights[i] : 0.f;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, focal_acc, nfocal, l1_acc, nl1, w,
                       out, factors);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_centernet_loss_fwd(const float* heat, const float* gt, long n_heat, const float* regr, int Cr,
                                      const float* off, int Co, int N, int HW, const int64_t* inds, const uint8_t* mask,
                                      const float* target, int K, int tstride, int toff_r, int toff_o,
                                      const float* l1_weights, float* g_heat, float* g_regr, float* g_off,
                                      double* focal_acc, float* out, float* factors, void* stream) {
    if (n_heat < 1 || K < 1 || N < 1 || g_off != g_regr + (long)N * Cr * HW) return SCD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long nz = (long)N * (Cr + Co) * HW;
    hipLaunchKernelGGL(centernet_loss_a_kernel, dim3(ew_blocks(std::max(n_heat, nz))), dim3(256), 0, st, heat, gt, n_heat,
                       g_heat, focal_acc, g_regr, nz);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    LossFin w;
    for (int i = 0; i < 8; ++i) w.l1w[i] = i < 2 ? l1_weights[i] : 0.f;
    L1Term t0{regr, g_regr, Cr, toff_r}, t1{off, g_off, Co, toff_o};
    hipLaunchKernelGGL(centernet_loss_b_kernel, dim3(1), dim3(1024), 0, st, N, HW, inds, mask, target, K, tstride, t0, t1,
                       focal_acc, w, out, factors);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_centernet_loss_bwd_scale(float* g_heat, long n_heat, int N, int HW, const int64_t* inds, int K,
                                            float* g_regr, int Cr, float* g_off, int Co, const float* factors,
                                            const float* go, void* stream) {
    hipLaunchKernelGGL(centernet_loss_scale_kernel, dim3(ew_blocks(n_heat)), dim3(256), 0, (hipStream_t)stream, g_heat,
                       n_heat, N, HW, inds, K, g_regr, Cr, g_off, Co, factors, go);
    SCD_RETURN_LAUNCH();
}

// Keep map of the pixels a CenterNet loss gathers (inds[n][k], all K slots): one workgroup, the previous call's
// pixels (prev, flattened n*HW + p; -1 = none) cleared first, then the new ones set and remembered, so the persistent
// map needs no full-size memset per step.
__global__ __launch_bounds__(1024) void heads_keep_map_kernel(const int64_t* inds, int N, int K, int HW, int64_t* prev,
                                                              int nprev, uint8_t* keep) {
    for (int i = threadIdx.x; i < nprev; i += blockDim.x) {
        const int64_t q = prev[i];
        if (q >= 0) keep[q] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N * K; i += blockDim.x) {
        const int n = i / K;
        const int64_t v = inds[i];
        const int64_t q = (v >= 0 && v < HW) ? (int64_t)n * HW + v : -1;
        if (q >= 0) keep[q] = 1;
        prev[i] = q;
    }
    for (int i = N * K + threadIdx.x; i < nprev; i += blockDim.x) prev[i] = -1;
}

extern "C" int scd_heads_keep_map(const int64_t* inds, int N, int K, int HW, int64_t* prev, int nprev, uint8_t* keep,
                                  void* stream) {
    if (N < 1 || K < 1 || HW < 1 || nprev < N * K) return SCD_ERR_ARG;
    hipLaunchKernelGGL(heads_keep_map_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, inds, N, K, HW, prev, nprev,
                       keep);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_scale_by_device(float* g, long n, const float* factors, int idx, const float* go, void* stream) {
    hipLaunchKernelGGL(scale_by_device_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, n, factors, idx,
                       go);
    SCD_RETURN_LAUNCH();
}

extern "C" size_t scd_decode_workspace(int N, int HW) { return (size_t)N * HW * sizeof(float); }

extern "C" int scd_decode_topk(const float* heat, int N, int H, int W, int K, const float* offset, int od_off,
                               const float* regr, int od_regr, float* scores, int64_t* inds, int64_t* ys, int64_t* xs,
                               float* off_out, float* regr_out, void* workspace, void* stream) {
    if (K < 1 || K > 1024 || K > H * W) return SCD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* t = (float*)workspace;
    hipLaunchKernelGGL(nms_kernel<NmsSigmoid>, dim3(ew_blocks((long)N * H * W)), dim3(256), 0, st, heat, (long)N, H, W, 3,
                       t);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(decode_select_kernel, dim3(N), dim3(1024), 0, st, t, H * W, W, K, offset, od_off, regr, od_regr,
                       scores, inds, ys, xs, off_out, regr_out);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_corner_pairs(const float* tl_scores, const int64_t* tl_inds, const int64_t* tl_ys,
                                const int64_t* tl_xs, const float* br_scores, const int64_t* br_inds,
                                const int64_t* br_ys, const int64_t* br_xs, const float* tl_tag, const float* br_tag,
                                int N, int K, int HW, float threshold, int D, float* det, int* nvalid, void* stream) {
    if (!tl_scores || !tl_inds || !tl_ys || !tl_xs || !br_scores || !br_inds || !br_ys || !br_xs || !tl_tag || !br_tag ||
        !det || !nvalid)
        return SCD_ERR_ARG;
    if (N < 1 || K < 1 || K > PAIR_MAXK || HW < 1 || D < 1 || D > 1024 || D > K * K) return SCD_ERR_ARG;
    hipLaunchKernelGGL(corner_pairs_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, tl_scores, tl_inds, tl_ys, tl_xs,
                       br_scores, br_inds, br_ys, br_xs, tl_tag, br_tag, K, HW, threshold, D, det, nvalid);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_corner_ae_fwd(const float* tl_tag, const float* br_tag, int N, int HW, const int64_t* tl_inds,
                                 const int64_t* br_inds, const uint8_t* valid, int K, float w_pull, float w_push,
                                 double* focal_acc, int nfocal, double* ae_acc, float* gs_tl, float* gs_br, float* out,
                                 float* factors, void* stream) {
    if (!tl_tag || !br_tag || !tl_inds || !br_inds || !valid || !focal_acc || !ae_acc || !gs_tl || !gs_br || !out ||
        !factors)
        return SCD_ERR_ARG;
    if (N < 1 || HW < 1 || (long)N * HW >= (1L << 31) || K < 1 || K > AE_MAXK || nfocal < 0) return SCD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(corner_ae_fwd_kernel, dim3(N), dim3(AE_THREADS), 0, st, tl_tag, br_tag, HW, tl_inds, br_inds,
                       valid, K, w_pull, w_push, ae_acc, gs_tl, gs_br);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(corner_ae_finalize_kernel, dim3(1), dim3(64), 0, st, focal_acc, nfocal, ae_acc, N, w_pull, w_push,
                       out, factors);
    SCD_RETURN_LAUNCH();
}

extern "C" int scd_corner_ae_bwd(const float* gs_tl, const float* gs_br, int N, int HW, const int64_t* tl_inds,
                                 const int64_t* br_inds, const uint8_t* valid, int K, const float* go, float* g_tl,
                                 float* g_br, void* stream) {
    if (!gs_tl || !gs_br || !tl_inds || !br_inds || !valid || !g_tl || !g_br) return SCD_ERR_ARG;
    if (N < 1 || N > 65535 || HW < 1 || (long)N * HW >= (1L << 31) || K < 1 || K > AE_MAXK) return SCD_ERR_ARG;
    const int slices = std::max(1, std::min(64, cdiv(HW, 256)));
    hipLaunchKernelGGL(corner_ae_bwd_kernel, dim3(slices, N), dim3(256), 0, (hipStream_t)stream, gs_tl, gs_br, tl_inds,
                       br_inds, valid, K, HW, go, g_tl, g_br);
    SCD_RETURN_LAUNCH();
}
