// Risk-group stratification: the log-rank sums and the Kaplan-Meier curves of R rows (bootstrap resamples = integer weights,
// label permutations / cut points = group bits) over ONE cohort, whose sort by time and tie blocks every row shares.
//
// One wavefront per row, SR_ROWS rows per workgroup, no LDS and no barrier: a wave walks the sorted samples 64 per trip.
//   sweep 1  the row's totals N = sum w, N1 = sum w g (any order: integers);
//   sweep 2  ascending. Four inclusive integer wave scans (w, w g, w e, w e g) with a carry between trips. The lane that holds the LAST
//            sample of a tie block forms the block's term: the scans at the previous block end (found with a ballot, fetched with one
//            shuffle each, or the carried values when that end lies in an earlier trip) give d = the block's event weight and
//            n = N - (weight before the block) at risk, and their group-1 parts. Every count is an exact integer below 2^31.
//            The curves are three inclusive PRODUCT scans of the blocks' factors (n - d) / n with a carried running product; a query
//            time takes the product at the last block at or before it (ws[k] = number of queries before sorted sample k, made by a
//            prologue launch; the lane of sample k owns the queries [ws[k], ws[k + 1]): up to SR_SERIAL of
//            them it stores alone, a longer run -- a dense plotting grid over a small cohort -- is stored by the whole wave).
// E1 and V are summed per lane in double over the trips and merged by a fixed butterfly: no atomics, the same bits every run, and a
// row's results depend on nothing but the row.
#include "common.h"
#include "../../include/advmil_hip.h"
#include <math.h>

constexpr int SR_ROWS = 4;                               // rows (wavefronts) per workgroup
constexpr int SR_SERIAL = 4;                             // queries between two sample times up to which their lane stores them alone

__device__ __forceinline__ uint32_t sr_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double sr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t sr_scan_add(uint32_t v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}
__device__ __forceinline__ double sr_scan_mul(double v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double u = __shfl_up(v, s, 64);
    if (lane >= s) v *= u;
  }
  return v;
}

// ws[k] = number of queries before stime[k] = the first q with at[q] >= stime[k]
__global__ __launch_bounds__(256) void logrank_query_kernel(const float* __restrict__ stime, int64_t n, const float* __restrict__ at, int Q,
                                                            int32_t* __restrict__ qlo) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const float t = stime[k];
  int lo = 0, hi = Q;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (at[mid] < t) lo = mid + 1; else hi = mid;
  }
  qlo[k] = lo;
}

__global__ __launch_bounds__(64 * SR_ROWS) void logrank_rows_kernel(const float* __restrict__ stime, const float* __restrict__ sevent,
                                                                    const int32_t* __restrict__ order, int64_t n,
                                                                    const uint8_t* __restrict__ groups, int64_t ldg,
                                                                    const int32_t* __restrict__ weights, int64_t ldw, int64_t R,
                                                                    const int32_t* __restrict__ qlo, int Q, long long* __restrict__ counts,
                                                                    double* __restrict__ sums, double* __restrict__ km,
                                                                    double* __restrict__ median) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * SR_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;                                    // (a whole wave: nothing below crosses waves)
  const uint8_t* g = groups + r * ldg;                   // ldg == 0: one row for all
  const int32_t* w = weights ? weights + r * ldw : nullptr;

  // ---- sweep 1: the totals the at-risk sums start from (the event totals fall out of sweep 2's carries) ----
  uint32_t tw = 0, tw1 = 0;
  for (int64_t k = lane; k < n; k += 64) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint64_t)n) o = 0;                         // a permutation is the caller's duty; no address outside a row in any case
    const uint32_t wk = w ? (uint32_t)w[o] : 1u;
    tw += wk; tw1 += g[o] != 0 ? wk : 0u;
  }
  tw = sr_wave_sum(tw); tw1 = sr_wave_sum(tw1);

  // ---- sweep 2: ascending over the tie blocks ----
  uint32_t cw = 0, cw1 = 0, ce = 0, ce1 = 0;             // the four sums through the previous trip ...
  uint32_t bw = 0, bw1 = 0, be = 0, be1 = 0;             // ... and at the last block end so far
  double S[3] = {1.0, 1.0, 1.0};                         // running products: group 0, group 1, pooled
  double med[3] = {INFINITY, INFINITY, INFINITY};
  bool found[3] = {false, false, false};
  double e1 = 0.0, var = 0.0;                            // this lane's share
  uint32_t nd = 0, nd2 = 0;
  double* kmr = km + r * 3 * (int64_t)Q;
  if (Q > 0) {                                           // queries before the first sample: the empty product
    const int first = qlo[0];
    for (int q = lane; q < first; q += 64) { kmr[q] = 1.0; kmr[(int64_t)Q + q] = 1.0; kmr[2 * (int64_t)Q + q] = 1.0; }
  }
#pragma unroll 1
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t k = base + lane;
    const bool in = k < n;
    float tk = 0.0f;
    bool end = false, ek = false, gk = false;
    uint32_t wk = 0;
    if (in) {
      tk = stime[k];
      end = (k + 1 == n) || (stime[k + 1] != tk);
      uint32_t o = (uint32_t)order[k];
      if (o >= (uint64_t)n) o = 0;
      wk = w ? (uint32_t)w[o] : 1u;
      gk = g[o] != 0;
      ek = sevent[k] != 0.0f;
    }
    const uint32_t pw = cw + sr_scan_add(wk, lane), pw1 = cw1 + sr_scan_add(gk ? wk : 0u, lane);
    const uint32_t pe = ce + sr_scan_add(ek ? wk : 0u, lane), pe1 = ce1 + sr_scan_add((ek && gk) ? wk : 0u, lane);
    const unsigned long long ends = __ballot(end);
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : lane;
    uint32_t qw = __shfl(pw, pl, 64), qw1 = __shfl(pw1, pl, 64), qe = __shfl(pe, pl, 64), qe1 = __shfl(pe1, pl, 64);
    if (!below) { qw = bw; qw1 = bw1; qe = be; qe1 = be1; }
    const uint32_t nn = tw - qw, n1 = tw1 - qw1, d = pe - qe, d1 = pe1 - qe1;
    const bool hit = end && d > 0;
    double f[3] = {1.0, 1.0, 1.0};
    if (hit) {
      const uint32_t n0 = nn - n1, d0 = d - d1;
      const double dn = (double)nn, dn1 = (double)n1, dd = (double)d;
      e1 += dd * dn1 / dn;
      if (nn > 1) var += (dn1 / dn) * ((double)n0 / dn) * dd * ((dn - dd) / (dn - 1.0));
      if (d0) f[0] = (double)(n0 - d0) / (double)n0;
      if (d1) f[1] = (double)(n1 - d1) / dn1;
      f[2] = (double)(nn - d) / dn;
    }
    nd += (uint32_t)__popcll(__ballot(hit));
    nd2 += (uint32_t)__popcll(__ballot(hit && nn > 1));
    double s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[c] = S[c] * sr_scan_mul(f[c], lane);
      if (!found[c]) {
        const unsigned long long at_half = __ballot(in && s[c] <= 0.5);
        if (at_half) {
          med[c] = (double)__shfl(tk, __ffsll((long long)at_half) - 1, 64);
          found[c] = true;
        }
      }
    }
    if (Q > 0) {                                         // (uniform: the branch holds cross-lane operations)
      int qa = 0, qb = 0;
      if (in && k + 1 < n) { qa = qlo[k]; qb = qlo[k + 1]; }
      const bool wide = qb - qa > SR_SERIAL;             // a long run of queries between two times: the whole wave stores it
      if (!wide)
        for (int q = qa; q < qb; ++q) { kmr[q] = s[0]; kmr[(int64_t)Q + q] = s[1]; kmr[2 * (int64_t)Q + q] = s[2]; }
      unsigned long long todo = __ballot(wide);
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int a = __shfl(qa, src, 64), b = __shfl(qb, src, 64);
        const double v0 = __shfl(s[0], src, 64), v1 = __shfl(s[1], src, 64), v2 = __shfl(s[2], src, 64);
        for (int q = a + lane; q < b; q += 64) { kmr[q] = v0; kmr[(int64_t)Q + q] = v1; kmr[2 * (int64_t)Q + q] = v2; }
      }
    }
    cw = __shfl(pw, 63, 64); cw1 = __shfl(pw1, 63, 64); ce = __shfl(pe, 63, 64); ce1 = __shfl(pe1, 63, 64);
    if (ends) {
      const int hl = 63 - __clzll((long long)ends);
      bw = __shfl(pw, hl, 64); bw1 = __shfl(pw1, hl, 64); be = __shfl(pe, hl, 64); be1 = __shfl(pe1, hl, 64);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) S[c] = __shfl(s[c], 63, 64);
  }
  if (Q > 0)                                             // queries at or after the last sample: the whole product
    for (int q = qlo[n - 1] + lane; q < Q; q += 64) { kmr[q] = S[0]; kmr[(int64_t)Q + q] = S[1]; kmr[2 * (int64_t)Q + q] = S[2]; }
  e1 = sr_wave_sum(e1);
  var = sr_wave_sum(var);
  if (lane == 0) {
    long long* c = counts + r * 6;
    c[0] = ce1; c[1] = ce; c[2] = tw1; c[3] = tw; c[4] = nd; c[5] = nd2;
    sums[r * 2] = e1; sums[r * 2 + 1] = var;
    median[r * 3] = med[0]; median[r * 3 + 1] = med[1]; median[r * 3 + 2] = med[2];
  }
}

extern "C" size_t advmil_logrank_rows_workspace_bytes(int64_t n, int Q) {
  return (Q > 0 && n > 0) ? (size_t)n * sizeof(int32_t) : 0;
}

extern "C" int advmil_logrank_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const uint8_t* groups,
                                   int64_t ldg, const int32_t* weights, int64_t ldw, int R, const float* at, int Q, int64_t* counts,
                                   double* sums, double* km, double* median, void* ws, size_t ws_bytes, advmil_stream_t stream_) {
  if (!stime || !sevent || !order || !groups || !counts || !sums || !median) return ADVMIL_EINVAL;
  if (n < 1 || n > (1 << 20) || R < 1 || R > (1 << 20) || Q < 0 || Q > (1 << 16)) return ADVMIL_EINVAL;
  if ((ldg != 0 && ldg < n) || (weights && ldw < n)) return ADVMIL_EINVAL;
  if (Q > 0 && (!at || !km || !ws)) return ADVMIL_EINVAL;
  if (((uintptr_t)stime & 3) || ((uintptr_t)sevent & 3) || ((uintptr_t)order & 3) || ((uintptr_t)weights & 3) || ((uintptr_t)at & 3) ||
      ((uintptr_t)ws & 3))
    return ADVMIL_EINVAL;
  if (((uintptr_t)counts & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)km & 7) || ((uintptr_t)median & 7)) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_logrank_rows_workspace_bytes(n, Q)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  if (Q > 0) {
    hipLaunchKernelGGL(logrank_query_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, stime, n, at, Q, (int32_t*)ws);
    ADVMIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(logrank_rows_kernel, dim3((unsigned)((R + SR_ROWS - 1) / SR_ROWS)), dim3(64 * SR_ROWS), 0, stream, stime, sevent,
                     order, n, groups, ldg, weights, ldw, (int64_t)R, (const int32_t*)ws, Q, (long long*)counts, sums, km, median);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
