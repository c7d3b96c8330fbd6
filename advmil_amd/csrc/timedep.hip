// Time-dependent evaluation: the IPCW Brier score (Graf et al.) and the cumulative/dynamic AUC(t) (Uno et al., Hung & Chiang) of R rows
// (bootstrap resamples = integer weights) over ONE cohort at Q query times. The cohort's sort by time, its tie blocks, the split of the
// sorted order into candidates for cases [0, k_q) and controls [k_q, n) and every risk comparison are the same for all rows.
//
// Three launches on the caller's stream:
//   prologue  bend[k] = the last sorted sample of k's tie block, kq[q] = #{k: stime[k] <= at[q]} (binary searches, one thread each);
//   walk      one wavefront per row, TD_WALK_ROWS rows per workgroup, no LDS and no barrier, 64 sorted samples per trip, the walk of
//             strat.hip: inclusive integer scans of w and w e with a carry, and at the lane that holds the LAST sample of a tie block
//             n(u), d(u), c(u) as exact integers. Two inclusive PRODUCT scans with a carried running product give G (censoring
//             Kaplan-Meier, events before censorings at a tied time) and S_KM at every block end. G goes to the workspace at the block
//             ends (the pair pass reads G(y_k) at bend[k]); the queries whose k_q - 1 lies in the trip take both products from that
//             lane by one shuffle each (kq ascends with at, so a wave-uniform cursor walks them once);
//   pairs     one workgroup of TD_T threads per (chunk of TD_R rows, query time). Controls: thread-strided, B and N_ctrl. Cases:
//             rounds of TD_T sorted samples, one per thread; the controls' risks and their TD_R weights are staged in LDS TD_T at a
//             time and every thread walks them (uniform addresses: broadcasts). The comparison 2[r_i > r_j] + [r_i = r_j] is formed
//             once per pair and reused by the chunk's rows: K += (w_j & mask) << shift, two integer instructions per pair and row.
//             K_i <= 2 N_ctrl < 2^32 is exact in 32 bits. The case then adds w_i / G(y_i) times 1, S^2 and K_i / 2 to its thread's
//             double sums; a fixed butterfly and a fixed merge of the four waves end the workgroup.
// No atomics anywhere; which thread adds which term in which order depends on n, k_q and the thread index only, never on R or on the
// row's place in the batch: a row of a batch has the bits of the one-row call, run after run.
#include "common.h"
#include "../../include/advmil_hip.h"

constexpr int TD_WALK_ROWS = 4;                          // rows (wavefronts) per workgroup of the walk
constexpr int TD_T = 256;                                // threads of a pair-pass workgroup = cases per round = controls per LDS tile
constexpr int TD_R = 8;                                  // rows a pair-pass workgroup carries

__device__ __forceinline__ uint32_t td_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double td_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t td_scan_add(uint32_t v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}
__device__ __forceinline__ double td_scan_mul(double v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double u = __shfl_up(v, s, 64);
    if (lane >= s) v *= u;
  }
  return v;
}

// threads [0, n): bend[k] = (the first k' with stime[k'] > stime[k]) - 1; threads [n, n + Q): kq[q] = the first k with stime[k] > at[q]
__global__ __launch_bounds__(256) void ipcw_prologue_kernel(const float* __restrict__ stime, int n, const float* __restrict__ at, int Q,
                                                            int32_t* __restrict__ bend, int32_t* __restrict__ kq) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n + Q) return;
  const float t = i < n ? stime[i] : at[i - n];
  int lo = i < n ? i + 1 : 0, hi = n;                    // (a block ends at or after its own sample)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (stime[mid] > t) hi = mid; else lo = mid + 1;
  }
  if (i < n) bend[i] = lo - 1; else kq[i - n] = lo;
}

__global__ __launch_bounds__(64 * TD_WALK_ROWS) void ipcw_walk_kernel(const float* __restrict__ stime, const float* __restrict__ sevent,
                                                                      const int32_t* __restrict__ order, int n,
                                                                      const int32_t* __restrict__ weights, int64_t ldw, int64_t R,
                                                                      const int32_t* __restrict__ kq, int Q, double* __restrict__ Gy,
                                                                      long long* __restrict__ rowcnt, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * TD_WALK_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;                                    // (a whole wave: nothing below crosses waves)
  const int32_t* w = weights ? weights + r * ldw : nullptr;
  double* gr = Gy + r * (int64_t)n;
  double* sr = sums + r * 6 * (int64_t)Q;

  // ---- sweep 1: the total the at-risk counts start from ----
  uint32_t tw = 0;
  for (int k = lane; k < n; k += 64) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint32_t)n) o = 0;                         // a permutation is the caller's duty; no address outside a row in any case
    tw += w ? (uint32_t)w[o] : 1u;
  }
  tw = td_wave_sum(tw);

  // ---- the queries before the first sample: the empty products ----
  int qc = 0;                                            // cursor: the queries [0, qc) are stored (wave-uniform)
  for (;;) {
    const int q = qc + lane;
    const bool hit = q < Q && kq[q] == 0;
    if (hit) { sr[(int64_t)q * 6 + 2] = 1.0; sr[(int64_t)q * 6 + 3] = 1.0; }
    const int c = __popcll(__ballot(hit));
    qc += c;
    if (c < 64) break;
  }

  // ---- sweep 2: ascending over the tie blocks ----
  uint32_t cw = 0, ce = 0;                               // the two sums through the previous trip ...
  uint32_t bw = 0, be = 0;                               // ... and at the last block end so far
  double PG = 1.0, PS = 1.0;                             // running products
#pragma unroll 1
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool in = k < n;
    bool end = false, ek = false;
    uint32_t wk = 0;
    if (in) {
      const float tk = stime[k];
      end = (k + 1 == n) || (stime[k + 1] != tk);
      uint32_t o = (uint32_t)order[k];
      if (o >= (uint32_t)n) o = 0;
      wk = w ? (uint32_t)w[o] : 1u;
      ek = sevent[k] != 0.0f;
    }
    const uint32_t pw = cw + td_scan_add(wk, lane), pe = ce + td_scan_add(ek ? wk : 0u, lane);
    const unsigned long long ends = __ballot(end);
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : lane;
    uint32_t qw = __shfl(pw, pl, 64), qe = __shfl(pe, pl, 64);
    if (!below) { qw = bw; qe = be; }
    double fg = 1.0, fs = 1.0;
    if (end) {
      const uint32_t nn = tw - qw, d = pe - qe, c = (pw - qw) - d;     // at risk, events and censorings of the block
      if (d) fs = (double)(nn - d) / (double)nn;
      if (c) fg = (double)(nn - d - c) / (double)(nn - d);
    }
    const double sg = PG * td_scan_mul(fg, lane), ss = PS * td_scan_mul(fs, lane);
    if (end) gr[k] = sg;
    // the queries whose last sample at or before them lies in this trip (uniform loop: it holds cross-lane operations)
    for (;;) {
      const int q = qc + lane;
      const int idx = q < Q ? kq[q] - 1 - base : 64;     // >= 0: everything before `base` is stored
      const bool hit = idx < 64;
      const int src = hit ? idx : 0;
      const double vg = __shfl(sg, src, 64), vs = __shfl(ss, src, 64);
      if (hit) { sr[(int64_t)q * 6 + 2] = vg; sr[(int64_t)q * 6 + 3] = vs; }
      const int c = __popcll(__ballot(hit));
      qc += c;
      if (c < 64) break;
    }
    cw = __shfl(pw, 63, 64); ce = __shfl(pe, 63, 64);
    if (ends) {
      const int hl = 63 - __clzll((long long)ends);
      bw = __shfl(pw, hl, 64); be = __shfl(pe, hl, 64);
    }
    PG = __shfl(sg, 63, 64); PS = __shfl(ss, 63, 64);
  }
  if (lane == 0) { rowcnt[r * 2] = tw; rowcnt[r * 2 + 1] = ce; }
}

__global__ __launch_bounds__(TD_T) void ipcw_pairs_kernel(const float* __restrict__ sevent, const int32_t* __restrict__ order, int n,
                                                          const int32_t* __restrict__ weights, int64_t ldw, int64_t R, int Q,
                                                          const float* __restrict__ surv, int64_t lds, const float* __restrict__ risk,
                                                          int64_t ldr, int risk_cols, const double* __restrict__ Gy,
                                                          const int32_t* __restrict__ bend, const int32_t* __restrict__ kq,
                                                          long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ float s_rho[TD_T];
  __shared__ uint32_t s_w[TD_T][TD_R];
  __shared__ double s_sum[TD_T / 64][4 * TD_R];
  __shared__ uint32_t s_cnt[TD_T / 64][2 * TD_R];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int q = blockIdx.y;
  const int64_t b0 = (int64_t)blockIdx.x * TD_R;
  const int k0 = kq[q];                                  // sorted samples [0, k0): time <= at[q]; [k0, n): the controls
  // past the last row the last row is read again (and its sums dropped), so the walks need no row guard
  int64_t row[TD_R];
  const int32_t* wr[TD_R];
#pragma unroll
  for (int r = 0; r < TD_R; ++r) {
    row[r] = b0 + r < R ? b0 + r : R - 1;
    wr[r] = weights ? weights + row[r] * ldw : nullptr;
  }
  const int64_t rcol = risk_cols == 1 ? 0 : q;
  double A[TD_R], B[TD_R], Wc[TD_R], C[TD_R];
  uint32_t ncase[TD_R], nctrl[TD_R];
#pragma unroll
  for (int r = 0; r < TD_R; ++r) { A[r] = 0.0; B[r] = 0.0; Wc[r] = 0.0; C[r] = 0.0; ncase[r] = 0; nctrl[r] = 0; }

  // ---- controls: N_ctrl and B ----
  for (int k = k0 + t; k < n; k += TD_T) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint32_t)n) o = 0;
    double u2 = 0.0;
    if (surv) {
      const double u = 1.0 - (double)surv[(int64_t)o * lds + q];
      u2 = u * u;
    }
#pragma unroll
    for (int r = 0; r < TD_R; ++r) {
      const uint32_t wj = wr[r] ? (uint32_t)wr[r][o] : 1u;
      nctrl[r] += wj;
      B[r] += (double)wj * u2;
    }
  }

  // ---- cases: rounds of TD_T sorted samples, one per thread ----
#pragma unroll 1
  for (int cb = 0; cb < k0; cb += TD_T) {
    const int k = cb + t;
    const bool is_case = k < k0 && sevent[k] != 0.0f;
    uint32_t o = is_case ? (uint32_t)order[k] : 0u;
    if (o >= (uint32_t)n) o = 0;
    uint32_t K[TD_R];
#pragma unroll
    for (int r = 0; r < TD_R; ++r) K[r] = 0;
    if (risk) {                                          // (uniform: the branch holds barriers)
      const float ri = is_case ? risk[(int64_t)o * ldr + rcol] : 0.0f;
#pragma unroll 1
      for (int j0 = k0; j0 < n; j0 += TD_T) {
        __syncthreads();                                 // the previous tile is consumed
        const int j = j0 + t;
        if (j < n) {
          uint32_t oj = (uint32_t)order[j];
          if (oj >= (uint32_t)n) oj = 0;
          s_rho[t] = risk[(int64_t)oj * ldr + rcol];
#pragma unroll
          for (int r = 0; r < TD_R; ++r) s_w[t][r] = wr[r] ? (uint32_t)wr[r][oj] : 1u;
        }
        __syncthreads();
        const int len = n - j0 < TD_T ? n - j0 : TD_T;
        if (is_case) {
#pragma unroll 4
          for (int jj = 0; jj < len; ++jj) {
            const float rj = s_rho[jj];
            const bool gt = ri > rj;
            const uint32_t mask = (gt || ri == rj) ? 0xFFFFFFFFu : 0u, shift = gt ? 1u : 0u;
#pragma unroll
            for (int r = 0; r < TD_R; ++r) K[r] += (s_w[jj][r] & mask) << shift;
          }
        }
      }
    }
    if (is_case) {
      double s2 = 0.0;
      if (surv) {
        const double s = (double)surv[(int64_t)o * lds + q];
        s2 = s * s;
      }
      const int kb = bend[k];
#pragma unroll
      for (int r = 0; r < TD_R; ++r) {
        const uint32_t wi = wr[r] ? (uint32_t)wr[r][o] : 1u;
        if (wi) {
          const double ig = (double)wi / Gy[row[r] * (int64_t)n + kb];
          ncase[r] += wi;
          Wc[r] += ig;
          A[r] += ig * s2;
          C[r] += ig * (0.5 * (double)K[r]);
        }
      }
    }
  }

  // ---- the workgroup's sums: a butterfly per wave, then the waves in order ----
#pragma unroll
  for (int r = 0; r < TD_R; ++r) {
    A[r] = td_wave_sum(A[r]); B[r] = td_wave_sum(B[r]); Wc[r] = td_wave_sum(Wc[r]); C[r] = td_wave_sum(C[r]);
    ncase[r] = td_wave_sum(ncase[r]); nctrl[r] = td_wave_sum(nctrl[r]);
    if (lane == 0) {
      s_sum[wave][r] = A[r]; s_sum[wave][TD_R + r] = B[r]; s_sum[wave][2 * TD_R + r] = Wc[r]; s_sum[wave][3 * TD_R + r] = C[r];
      s_cnt[wave][r] = ncase[r]; s_cnt[wave][TD_R + r] = nctrl[r];
    }
  }
  __syncthreads();
  if (t < TD_R && b0 + t < R) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t c0 = 0, c1 = 0;
    for (int wv = 0; wv < TD_T / 64; ++wv) {
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] += s_sum[wv][s * TD_R + t];
      c0 += s_cnt[wv][t]; c1 += s_cnt[wv][TD_R + t];
    }
    if (c1 == 0) { v[0] = 0.0; v[2] = 0.0; v[3] = 0.0; } // no control: nothing is defined at this time; G may be 0 there
    const int64_t e = (b0 + t) * (int64_t)Q + q;
    counts[e * 2] = c0; counts[e * 2 + 1] = c1;
    sums[e * 6] = v[0]; sums[e * 6 + 1] = v[1]; sums[e * 6 + 4] = v[2]; sums[e * 6 + 5] = v[3];
  }
}

static bool td_shape_ok(int64_t n, int64_t R, int64_t Q) {
  return n >= 1 && n <= (1 << 16) && R >= 1 && R <= (1 << 20) && Q >= 1 && Q <= 4096;
}

extern "C" size_t advmil_ipcw_rows_workspace_bytes(int64_t n, int R, int Q) {
  if (!td_shape_ok(n, R, Q)) return 0;
  return (size_t)R * (size_t)n * sizeof(double) + (((size_t)n + (size_t)Q + 1) & ~(size_t)1) * sizeof(int32_t);
}

extern "C" int advmil_ipcw_rows_plan(int* walk_rows, int* walk_trip, int* pair_tile, int* pair_rows) {
  if (!walk_rows || !walk_trip || !pair_tile || !pair_rows) return ADVMIL_EINVAL;
  *walk_rows = TD_WALK_ROWS; *walk_trip = 64; *pair_tile = TD_T; *pair_rows = TD_R;
  return ADVMIL_OK;
}

extern "C" int advmil_ipcw_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights,
                                int64_t ldw, int R, const float* at, int Q, const float* surv, int64_t lds, const float* risk, int64_t ldr,
                                int risk_cols, int64_t* counts, int64_t* rowcnt, double* sums, void* ws, size_t ws_bytes,
                                advmil_stream_t stream_) {
  if (!stime || !sevent || !order || !at || !counts || !rowcnt || !sums || !ws) return ADVMIL_EINVAL;
  if (!td_shape_ok(n, R, Q)) return ADVMIL_EINVAL;
  if (weights && ldw < n) return ADVMIL_EINVAL;
  if (surv && lds < Q) return ADVMIL_EINVAL;
  if (risk && ((risk_cols != 1 && risk_cols != Q) || ldr < risk_cols)) return ADVMIL_EINVAL;
  if (((uintptr_t)stime & 3) || ((uintptr_t)sevent & 3) || ((uintptr_t)order & 3) || ((uintptr_t)weights & 3) || ((uintptr_t)at & 3) ||
      ((uintptr_t)surv & 3) || ((uintptr_t)risk & 3))
    return ADVMIL_EINVAL;
  if (((uintptr_t)counts & 7) || ((uintptr_t)rowcnt & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)ws & 7)) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_ipcw_rows_workspace_bytes(n, R, Q)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  double* Gy = (double*)ws;                              // [R, n]: G at the block ends of the sorted order
  int32_t* bend = (int32_t*)(Gy + (size_t)R * (size_t)n);
  int32_t* kq = bend + n;
  const int ni = (int)n;
  hipLaunchKernelGGL(ipcw_prologue_kernel, dim3((unsigned)((n + Q + 255) / 256)), dim3(256), 0, stream, stime, ni, at, Q, bend, kq);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(ipcw_walk_kernel, dim3((unsigned)((R + TD_WALK_ROWS - 1) / TD_WALK_ROWS)), dim3(64 * TD_WALK_ROWS), 0, stream, stime,
                     sevent, order, ni, weights, ldw, (int64_t)R, (const int32_t*)kq, Q, Gy, (long long*)rowcnt, sums);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(ipcw_pairs_kernel, dim3((unsigned)((R + TD_R - 1) / TD_R), (unsigned)Q), dim3(TD_T), 0, stream, sevent, order, ni,
                     weights, ldw, (int64_t)R, Q, surv, lds, risk, ldr, risk_cols, (const double*)Gy, (const int32_t*)bend,
                     (const int32_t*)kq, (long long*)counts, sums);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
