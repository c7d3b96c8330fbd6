// Concordance index counts for right-censored data (eval/cindex.py:79-143 of the reference, the scikit-survival estimator with
// unit weights): all O(n^2) pair tests on the device, integer counters (bit-exact against the reference's python loops).
#include "common.h"
#include "../../include/advmil_hip.h"

// out[0..5] = concordant, discordant, tied_risk, tied_time, comparable, events_with_entry
__global__ __launch_bounds__(256) void cindex_counts_kernel(const float* __restrict__ time, const float* __restrict__ event,
                                                            const float* __restrict__ est, int64_t n, float tied_tol,
                                                            unsigned long long* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (!(event[i] != 0.0f)) return;                        // only samples with an event anchor comparable pairs (cindex.py:94)
  const float ti = time[i], ei = est[i];
  unsigned long long con = 0, dis = 0, tie = 0, tt = 0, comp = 0, ge = 0;
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    if (j == i) continue;
    const float tj = time[j];
    const bool later = tj > ti;
    const bool same_cens = (tj == ti) && !(event[j] != 0.0f);     // censored at the same time (cindex.py:92-101)
    ge += (tj >= ti);
    if (later || same_cens) {
      ++comp;
      tt += same_cens;
      const float ej = est[j];
      if (fabsf(ej - ei) <= tied_tol) ++tie;                     // cindex.py:125
      else if (ej < ei) ++con;                                   // cindex.py:128
      else ++dis;
    }
  }
  __shared__ unsigned long long red[6][256];
  red[0][threadIdx.x] = con; red[1][threadIdx.x] = dis; red[2][threadIdx.x] = tie;
  red[3][threadIdx.x] = tt;  red[4][threadIdx.x] = comp; red[5][threadIdx.x] = ge;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int q = 0; q < 6; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if (red[q][0]) atomicAdd(out + q, red[q][0]);
    // the reference registers an event unless it is the unique sample with the largest time (cindex.py:85-104)
    if (red[5][0]) atomicAdd(out + 5, 1ULL);
  }
}

extern "C" int advmil_cindex_counts(const float* time, const float* event, const float* estimate, int64_t n, float tied_tol,
                                    int64_t* out6, advmil_stream_t stream_) {
  if (!time || !event || !estimate || !out6 || n <= 0 || n > 0x7fffffff) return ADVMIL_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t err = hipMemsetAsync(out6, 0, 6 * sizeof(int64_t), stream);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(cindex_counts_kernel, dim3((unsigned)n), dim3(256), 0, stream, time, event, estimate, n, tied_tol,
                     (unsigned long long*)out6);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Weighted counts: B resamples (rows of multiplicities over the same n samples) x M estimate rows in one pass over the pairs.
// The class of a pair (i, j) does not depend on the resample; only its weight w_i * w_j does. One workgroup takes one event
// anchor i and one chunk of CB_R resamples: a thread classifies its j against the anchor once, then walks the chunk with the
// CB_R accumulators of each class in registers (weights[b, j] is read coalesced along j). The sums over j are multiplied by w_i
// once, after the workgroup's reduction. All arithmetic is integer in 64-bit counters: any accumulation order gives the same bits.
//
// j == i needs no special case: the anchor is an event, so it is neither later than itself nor censored at its own time; it does
// count in sum_j w_j [t_j >= t_i], which is what "has an entry" asks for (the copies of a sample are entries of each other).
constexpr int CB_T = 256;                   // threads of a workgroup = stride of the walk over j
constexpr int CB_R = 8;                     // resamples per chunk
constexpr int CB_MAX_CHUNK_BLOCKS = 4096;   // gridDim.y; chunks beyond it are taken by a stride loop
constexpr int CB_K0 = 3 * CB_R;             // sums that do not depend on the estimate: comparable | tied_time | at or after
constexpr int CB_K1 = 2 * CB_R;             // sums of one estimate row: concordant | tied_risk (discordant = comparable - both)

// Sum over the workgroup of K = classes x CB_R values per thread; value k ends in tot[k], readable behind the closing barrier. One
// class at a time: every thread stores its CB_R sums, then the 32 threads of resample r each fold CB_T / 32 of them and finish in
// five shuffle steps. The next call writes `buf` only, before its first barrier, so readers of tot need no barrier of their own.
template <int K>
__device__ __forceinline__ void cb_block_sum(const unsigned long long (&v)[K], unsigned long long (&buf)[CB_R][CB_T],
                                             unsigned long long (&tot)[CB_K0]) {
  static_assert(K % CB_R == 0 && K <= CB_K0 && CB_T == 32 * CB_R, "32 threads fold one resample");
  const int r = threadIdx.x >> 5, l = threadIdx.x & 31;
#pragma unroll
  for (int q = 0; q < K / CB_R; ++q) {
#pragma unroll
    for (int rr = 0; rr < CB_R; ++rr) buf[rr][threadIdx.x] = v[q * CB_R + rr];
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < CB_T / 32; ++k) s += buf[r][l + 32 * k];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) tot[q * CB_R + r] = s;
    __syncthreads();
  }
}

// One walk over j for anchor i. SHARED: the classes that do not depend on the estimate (once per chunk); else those of row `em`.
template <bool SHARED>
__device__ __forceinline__ void cb_walk(const float* __restrict__ time, const float* __restrict__ event, const float* __restrict__ em,
                                        const int32_t* (&wr)[CB_R], int64_t i, int64_t n, float ti, float tied_tol,
                                        unsigned long long (&acc)[SHARED ? CB_K0 : CB_K1]) {
  const float ei = SHARED ? 0.0f : em[i];
#pragma unroll
  for (int k = 0; k < (SHARED ? CB_K0 : CB_K1); ++k) acc[k] = 0;
#pragma unroll 1
  for (int64_t j = threadIdx.x; j < n; j += CB_T) {
    const float tj = time[j];
    const bool later = tj > ti;
    const bool same_cens = (tj == ti) && !(event[j] != 0.0f);        // censored at the same time (cindex.py:92-101)
    const bool cmp = later || same_cens;
    if (SHARED) {
      if (!(tj >= ti)) continue;
#pragma unroll
      for (int r = 0; r < CB_R; ++r) {
        const unsigned long long wj = (uint32_t)wr[r][j];
        acc[r] += cmp ? wj : 0ULL;
        acc[CB_R + r] += same_cens ? wj : 0ULL;
        acc[2 * CB_R + r] += wj;
      }
    } else {
      if (!cmp) continue;
      const float ej = em[j];
      const bool tie = fabsf(ej - ei) <= tied_tol;                   // cindex.py:125
      const bool con = !tie && ej < ei;                              // cindex.py:128
#pragma unroll
      for (int r = 0; r < CB_R; ++r) {
        const unsigned long long wj = (uint32_t)wr[r][j];
        acc[r] += con ? wj : 0ULL;
        acc[CB_R + r] += tie ? wj : 0ULL;
      }
    }
  }
}

// out[m, b, 0..5]. Slots 3..5 do not depend on m: they are summed in row m = 0 only and copied by cindex_weighted_finish_kernel.
__global__ __launch_bounds__(CB_T, 4) void cindex_counts_weighted_kernel(const float* __restrict__ time, const float* __restrict__ event,
                                                                         const float* __restrict__ est, int64_t lde, int M,
                                                                         const int32_t* __restrict__ w, int64_t ldw, int64_t B, int64_t n,
                                                                         float tied_tol, unsigned long long* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (!(event[i] != 0.0f)) return;                       // only samples with an event anchor comparable pairs (cindex.py:94)
  const float ti = time[i];
  __shared__ unsigned long long buf[CB_R][CB_T];
  __shared__ unsigned long long tot[CB_K0];
  const int64_t chunks = (B + CB_R - 1) / CB_R;
  const int r_own = threadIdx.x;                         // behind a reduction, threads 0 .. CB_R - 1 own one resample each
  for (int64_t c = blockIdx.y; c < chunks; c += gridDim.y) {
    const int64_t b0 = c * CB_R;
    // past the last resample the last row is read again (and its sums dropped), so the walks need no row guard
    const int32_t* wr[CB_R];
#pragma unroll
    for (int r = 0; r < CB_R; ++r) wr[r] = w + (b0 + r < B ? b0 + r : B - 1) * ldw;
    const bool owner = r_own < CB_R && b0 + r_own < B;
    const unsigned long long wi = owner ? (unsigned long long)(uint32_t)w[(b0 + r_own) * ldw + i] : 0ULL;
    unsigned long long comp = 0;
    {
      unsigned long long acc[CB_K0];
      cb_walk<true>(time, event, est, wr, i, n, ti, tied_tol, acc);
      cb_block_sum<CB_K0>(acc, buf, tot);
      if (owner && wi) {
        unsigned long long* o = out + (b0 + r_own) * 8;
        comp = tot[r_own];
        const unsigned long long tt = tot[CB_R + r_own];
        if (tt) atomicAdd(o + 3, wi * tt);
        if (comp) atomicAdd(o + 4, wi * comp);
        // an event copy has an entry unless it is the only copy of anything at or after its time (cindex.py:85-104)
        if (tot[2 * CB_R + r_own] > 1) atomicAdd(o + 5, wi);
      }
    }
    for (int m = 0; m < M; ++m) {
      unsigned long long acc[CB_K1];
      cb_walk<false>(time, event, est + (int64_t)m * lde, wr, i, n, ti, tied_tol, acc);
      cb_block_sum<CB_K1>(acc, buf, tot);
      if (owner && wi) {
        unsigned long long* o = out + ((int64_t)m * B + b0 + r_own) * 8;
        const unsigned long long con = tot[r_own], tie = tot[CB_R + r_own], dis = comp - con - tie;
        if (con) atomicAdd(o + 0, wi * con);
        if (dis) atomicAdd(o + 1, wi * dis);
        if (tie) atomicAdd(o + 2, wi * tie);
      }
    }
  }
}

// One workgroup per resample b: slots 6 (event copies) and 7 (size) of every row m, and slots 3..5 of row 0 copied to rows m > 0.
__global__ __launch_bounds__(CB_T) void cindex_weighted_finish_kernel(const float* __restrict__ event, const int32_t* __restrict__ w,
                                                                      int64_t ldw, int64_t B, int64_t n, int M,
                                                                      unsigned long long* __restrict__ out) {
  const int64_t b = blockIdx.x;
  const int32_t* wb = w + b * ldw;
  unsigned long long ev = 0, sz = 0;
  for (int64_t j = threadIdx.x; j < n; j += CB_T) {
    const unsigned long long wj = (uint32_t)wb[j];
    sz += wj;
    ev += event[j] != 0.0f ? wj : 0ULL;
  }
  __shared__ unsigned long long red[2][CB_T];
  red[0][threadIdx.x] = ev; red[1][threadIdx.x] = sz;
  __syncthreads();
  for (int s = CB_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
    __syncthreads();
  }
  for (int m = threadIdx.x; m < M; m += CB_T) {
    unsigned long long* o = out + ((int64_t)m * B + b) * 8;
    if (m > 0) { o[3] = out[b * 8 + 3]; o[4] = out[b * 8 + 4]; o[5] = out[b * 8 + 5]; }
    o[6] = red[0][0]; o[7] = red[1][0];
  }
}

extern "C" int advmil_cindex_counts_weighted_plan(int* row_tile, int* resample_chunk, int* max_chunk_blocks) {
  if (!row_tile || !resample_chunk || !max_chunk_blocks) return ADVMIL_EINVAL;
  *row_tile = CB_T; *resample_chunk = CB_R; *max_chunk_blocks = CB_MAX_CHUNK_BLOCKS;
  return ADVMIL_OK;
}

extern "C" int advmil_cindex_counts_weighted(const float* time, const float* event, const float* estimate, int64_t lde, int M,
                                             const int32_t* weights, int64_t ldw, int B, int64_t n, float tied_tol, int64_t* out,
                                             advmil_stream_t stream_) {
  if (!time || !event || !estimate || !weights || !out) return ADVMIL_EINVAL;
  if (n < 1 || n > (1 << 20) || B < 1 || B > (1 << 20) || M < 1 || M > 64 || lde < n || ldw < n) return ADVMIL_EINVAL;
  if (!(tied_tol >= 0.0f)) return ADVMIL_EINVAL;         // negative or NaN
  if (((uintptr_t)weights & 3) || ((uintptr_t)estimate & 3) || ((uintptr_t)out & 7)) return ADVMIL_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t err = hipMemsetAsync(out, 0, (size_t)M * B * 8 * sizeof(int64_t), stream);
  if (err != hipSuccess) return (int)err;
  const int64_t chunks = ((int64_t)B + CB_R - 1) / CB_R;
  const unsigned gy = (unsigned)(chunks < CB_MAX_CHUNK_BLOCKS ? chunks : CB_MAX_CHUNK_BLOCKS);
  hipLaunchKernelGGL(cindex_counts_weighted_kernel, dim3((unsigned)n, gy), dim3(CB_T), 0, stream, time, event, estimate, lde, M,
                     weights, ldw, (int64_t)B, n, tied_tol, (unsigned long long*)out);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(cindex_weighted_finish_kernel, dim3((unsigned)B), dim3(CB_T), 0, stream, event, weights, ldw, (int64_t)B, n, M,
                     (unsigned long long*)out);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
