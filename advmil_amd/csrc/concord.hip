// Concordance of R rows (bootstrap resamples = integer weights) over ONE cohort: the pair counts of Harrell's C and of Antolini's
// time-dependent concordance, and the sums of Uno's C at T truncation times (include/advmil_hip.h has the definitions). The cohort's
// sort by time, its tie blocks, which pairs are comparable and every comparison of two predictions are the same for all rows.
//
// Four launches on the caller's stream:
//   prologue  bend[k] = the last sorted sample of k's tie block (a binary search per thread);
//   walk      one wavefront per row, CC_WALK_ROWS rows per workgroup, 64 sorted samples per trip: the censoring Kaplan-Meier product G
//             at every tie-block end, into the workspace. It is the walk of timedep.hip RESTATED without the event product and the query
//             times (advmil_ipcw_rows is not touched): the same integer scans, the same product scan, so the same bits of G;
//   pairs     one workgroup of CC_T threads per (chunk of CC_R rows, tile of CC_T sorted samples = the cases, one per thread). The
//             controls come CC_T at a time through LDS: per control one 16-byte record (key, risk bits, sample index) and its CC_R
//             weights, every thread walks them (uniform addresses: broadcasts). With key_j = 2 bend[j] + [e_j = 0] the pair (i, j) is
//             comparable iff key_j > 2 bend[i]: one integer comparison. The comparisons are formed once per pair and reused by the
//             chunk's rows: K += w_j & mask. No comparable control lies before the case's tie block, so the walk over the controls starts
//             at the first sample of the tile's first block and the rest of the triangle is never visited. The surv source compares
//             surv[j, col[i]]: the column belongs to the CASE, so an element of the cases x controls block is used by one thread once and
//             LDS has nothing to share; the lanes of a wave hold consecutive sorted cases, whose columns ascend, so one load instruction
//             reads a short run of one row (the row pitch is the caller's). K_i is exact in 32 bits (K_i <= sum w < 2^31); sum_i w_i K_i
//             is exact in 64. The case then adds (w_i / G(y_i)^2) K_i to the double sums of every tau beyond its time; a fixed butterfly
//             per wave and a fixed merge of the four waves leave the tile's partial sums in the workspace;
//   reduce    one thread per (row, slot) adds the tiles' partials in ascending tile order and writes every output slot.
// No atomics anywhere; which thread adds which term in which order depends on n and the thread index only, never on R or on the row's
// place in the batch: a row of a batch has the bits of the one-row call, run after run.
#include "common.h"
#include "../../include/advmil_hip.h"

constexpr int CC_WALK_ROWS = 4;                          // rows (wavefronts) per workgroup of the walk
constexpr int CC_T = 256;                                // threads of a pair-pass workgroup = cases per tile = controls per LDS tile
constexpr int CC_R = 8;                                  // rows a pair-pass workgroup carries
constexpr int CC_MAXT = 8;                               // truncation times
// a tile's partial sums per row, 8-byte slots: 0 comp, 1-2 conc / tied (risk), 3-4 conc / tied (surv): sum_i w_i K_i (integers);
// 5 + t: weight of the cases before tau[t] with G = 0 (integer); 5 + T + 5 t + (0 ... 4): the five Uno sums of tau[t] (doubles)
__host__ __device__ constexpr int cc_slots(int T) { return 5 + 6 * T; }

__device__ __forceinline__ uint32_t cc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long cc_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t cc_scan_add(uint32_t v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}
__device__ __forceinline__ double cc_scan_mul(double v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double u = __shfl_up(v, s, 64);
    if (lane >= s) v *= u;
  }
  return v;
}

// bend[k] = (the first k' with stime[k'] > stime[k]) - 1
__global__ __launch_bounds__(256) void concord_prologue_kernel(const float* __restrict__ stime, int n, int32_t* __restrict__ bend) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const float t = stime[i];
  int lo = i + 1, hi = n;                                // (a block ends at or after its own sample)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (stime[mid] > t) hi = mid; else lo = mid + 1;
  }
  bend[i] = lo - 1;
}

__global__ __launch_bounds__(64 * CC_WALK_ROWS) void concord_walk_kernel(const float* __restrict__ stime, const float* __restrict__ sevent,
                                                                         const int32_t* __restrict__ order, int n,
                                                                         const int32_t* __restrict__ weights, int64_t ldw, int64_t R,
                                                                         int nrc, double* __restrict__ Gy, long long* __restrict__ rowcnt) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * CC_WALK_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;                                    // (a whole wave: nothing below crosses waves)
  const int32_t* w = weights ? weights + r * ldw : nullptr;
  double* gr = Gy + r * (int64_t)n;

  // ---- sweep 1: the total the at-risk counts start from ----
  uint32_t tw = 0;
  for (int k = lane; k < n; k += 64) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint32_t)n) o = 0;                         // a permutation is the caller's duty; no address outside a row in any case
    tw += w ? (uint32_t)w[o] : 1u;
  }
  tw = cc_wave_sum(tw);

  // ---- sweep 2: ascending over the tie blocks ----
  uint32_t cw = 0, ce = 0;                               // the two sums through the previous trip ...
  uint32_t bw = 0, be = 0;                               // ... and at the last block end so far
  double PG = 1.0;                                       // running product
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
    const uint32_t pw = cw + cc_scan_add(wk, lane), pe = ce + cc_scan_add(ek ? wk : 0u, lane);
    const unsigned long long ends = __ballot(end);
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : lane;
    uint32_t qw = __shfl(pw, pl, 64), qe = __shfl(pe, pl, 64);
    if (!below) { qw = bw; qe = be; }
    double fg = 1.0;
    if (end) {
      const uint32_t nn = tw - qw, d = pe - qe, c = (pw - qw) - d;     // at risk, events and censorings of the block
      if (c) fg = (double)(nn - d - c) / (double)(nn - d);
    }
    const double sg = PG * cc_scan_mul(fg, lane);
    if (end) gr[k] = sg;
    cw = __shfl(pw, 63, 64); ce = __shfl(pe, 63, 64);
    if (ends) {
      const int hl = 63 - __clzll((long long)ends);
      bw = __shfl(pw, hl, 64); be = __shfl(pe, hl, 64);
    }
    PG = __shfl(sg, 63, 64);
  }
  if (lane == 0) { rowcnt[r * nrc] = tw; rowcnt[r * nrc + 1] = ce; }
}

template <bool RISK, bool SURV>
__global__ __launch_bounds__(CC_T) void concord_pairs_kernel(const float* __restrict__ stime, const float* __restrict__ sevent,
                                                             const int32_t* __restrict__ order, int n, const int32_t* __restrict__ weights,
                                                             int64_t ldw, int64_t R, const float* __restrict__ risk,
                                                             const float* __restrict__ surv, int64_t lds, int Q,
                                                             const int32_t* __restrict__ col, const float* __restrict__ tau, int T,
                                                             const double* __restrict__ Gy, const int32_t* __restrict__ bend,
                                                             unsigned long long* __restrict__ part) {
  __shared__ int4 s_c[CC_T];                             // per control: key, risk bits, sample index
  __shared__ uint4 s_w[CC_T][CC_R / 4];
  __shared__ unsigned long long s_p[CC_T / 64][CC_R][cc_slots(CC_MAXT)];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ct = blockIdx.y, ntile = gridDim.y, nslot = cc_slots(T);
  const int64_t b0 = (int64_t)blockIdx.x * CC_R;
  const int cb = ct * CC_T;                              // < n by the grid
  // past the last row the last row is read again (and its sums dropped), so the walks need no row guard
  int64_t row[CC_R];
  const int32_t* wr[CC_R];
#pragma unroll
  for (int r = 0; r < CC_R; ++r) {
    row[r] = b0 + r < R ? b0 + r : R - 1;
    wr[r] = weights ? weights + row[r] * ldw : nullptr;
  }

  // ---- the case of this thread ----
  const int k = cb + t;
  const bool is_case = k < n && sevent[k] != 0.0f;
  uint32_t o = is_case ? (uint32_t)order[k] : 0u;
  if (o >= (uint32_t)n) o = 0;
  const int kb = is_case ? bend[k] : 0;
  const int key_i = 2 * kb;
  const float ti = is_case ? stime[k] : 0.0f;
  float ri = 0.0f, si = 0.0f;
  int64_t ci = 0;
  if (RISK && is_case) ri = risk[o];
  if (SURV && is_case) {
    int c = col[o];
    c = c < 0 ? 0 : (c >= Q ? Q - 1 : c);                // a column in [0, Q) is the caller's duty; no address outside a row in any case
    ci = c;
    si = surv[(int64_t)o * lds + ci];
  }
  // the first sample of the tile's first tie block: no comparable control lies before it
  int jstart = 0;
  {
    const float t0 = stime[cb];
    int lo = 0, hi = cb;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (stime[mid] < t0) lo = mid + 1; else hi = mid;
    }
    jstart = lo;
  }

  uint32_t Kc[CC_R], Kr1[CC_R], Kr2[CC_R], Ks1[CC_R], Ks2[CC_R];
#pragma unroll
  for (int r = 0; r < CC_R; ++r) { Kc[r] = 0; Kr1[r] = 0; Kr2[r] = 0; Ks1[r] = 0; Ks2[r] = 0; }

  if (__syncthreads_or(is_case ? 1 : 0)) {               // (uniform: the branch holds barriers)
#pragma unroll 1
    for (int j0 = jstart; j0 < n; j0 += CC_T) {
      __syncthreads();                                   // the previous tile is consumed
      const int j = j0 + t;
      if (j < n) {
        uint32_t oj = (uint32_t)order[j];
        if (oj >= (uint32_t)n) oj = 0;
        s_c[t] = make_int4(2 * bend[j] + (sevent[j] == 0.0f ? 1 : 0), RISK ? __float_as_int(risk[oj]) : 0, (int)oj, 0);
        uint32_t wv[CC_R];
#pragma unroll
        for (int r = 0; r < CC_R; ++r) wv[r] = wr[r] ? (uint32_t)wr[r][oj] : 1u;
#pragma unroll
        for (int r = 0; r < CC_R / 4; ++r) s_w[t][r] = make_uint4(wv[4 * r], wv[4 * r + 1], wv[4 * r + 2], wv[4 * r + 3]);
      }
      __syncthreads();
      const int len = n - j0 < CC_T ? n - j0 : CC_T;
      if (is_case) {
#pragma unroll 4
        for (int jj = 0; jj < len; ++jj) {
          const int4 c = s_c[jj];
          const bool cm = c.x > key_i;
          uint32_t wv[CC_R];
#pragma unroll
          for (int r = 0; r < CC_R / 4; ++r) {
            const uint4 q = s_w[jj][r];
            wv[4 * r] = q.x; wv[4 * r + 1] = q.y; wv[4 * r + 2] = q.z; wv[4 * r + 3] = q.w;
          }
          const uint32_t mc = cm ? 0xFFFFFFFFu : 0u;
#pragma unroll
          for (int r = 0; r < CC_R; ++r) Kc[r] += wv[r] & mc;
          if (RISK) {
            const float rj = __int_as_float(c.y);
            const uint32_t m1 = (cm && ri > rj) ? 0xFFFFFFFFu : 0u, m2 = (cm && ri == rj) ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int r = 0; r < CC_R; ++r) { Kr1[r] += wv[r] & m1; Kr2[r] += wv[r] & m2; }
          }
          if (SURV) {
            const float sj = surv[(int64_t)c.z * lds + ci];
            const uint32_t m1 = (cm && si < sj) ? 0xFFFFFFFFu : 0u, m2 = (cm && si == sj) ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int r = 0; r < CC_R; ++r) { Ks1[r] += wv[r] & m1; Ks2[r] += wv[r] & m2; }
          }
        }
      }
    }
  }

  // ---- the case's weight in every row: w_i for the counts, w_i / G(y_i)^2 for the Uno sums ----
  double ig2[CC_R];
  uint32_t zg[CC_R];
#pragma unroll
  for (int r = 0; r < CC_R; ++r) {
    const uint32_t wi = is_case ? (wr[r] ? (uint32_t)wr[r][o] : 1u) : 0u;
    ig2[r] = 0.0; zg[r] = 0;
    if (wi) {
      const double g = Gy[row[r] * (int64_t)n + kb];
      if (g > 0.0) ig2[r] = (double)wi / (g * g); else zg[r] = wi;
    }
    const unsigned long long w64 = wi;
    const unsigned long long v0 = cc_wave_sum(w64 * Kc[r]), v1 = cc_wave_sum(w64 * Kr1[r]), v2 = cc_wave_sum(w64 * Kr2[r]),
                             v3 = cc_wave_sum(w64 * Ks1[r]), v4 = cc_wave_sum(w64 * Ks2[r]);
    if (lane == 0) { s_p[wave][r][0] = v0; s_p[wave][r][1] = v1; s_p[wave][r][2] = v2; s_p[wave][r][3] = v3; s_p[wave][r][4] = v4; }
  }
#pragma unroll 1
  for (int q = 0; q < T; ++q) {
    const bool inc = is_case && ti < tau[q];
#pragma unroll
    for (int r = 0; r < CC_R; ++r) {
      const double f = inc ? ig2[r] : 0.0;
      const uint32_t z = cc_wave_sum(inc ? zg[r] : 0u);
      const double d0 = cc_wave_sum(f * (double)Kc[r]), d1 = cc_wave_sum(f * (double)Kr1[r]), d2 = cc_wave_sum(f * (double)Kr2[r]),
                   d3 = cc_wave_sum(f * (double)Ks1[r]), d4 = cc_wave_sum(f * (double)Ks2[r]);
      if (lane == 0) {
        unsigned long long* p = s_p[wave][r];
        p[5 + q] = z;
        p += 5 + T + 5 * q;
        p[0] = (unsigned long long)__double_as_longlong(d0); p[1] = (unsigned long long)__double_as_longlong(d1);
        p[2] = (unsigned long long)__double_as_longlong(d2); p[3] = (unsigned long long)__double_as_longlong(d3);
        p[4] = (unsigned long long)__double_as_longlong(d4);
      }
    }
  }
  __syncthreads();
  // ---- the tile's partials: the waves in order ----
  for (int idx = t; idx < CC_R * nslot; idx += CC_T) {
    const int r = idx / nslot, slot = idx - r * nslot;
    if (b0 + r >= R) break;
    unsigned long long v;
    if (slot < 5 + T) {
      v = 0;
      for (int wv = 0; wv < CC_T / 64; ++wv) v += s_p[wv][r][slot];
    } else {
      double d = 0.0;
      for (int wv = 0; wv < CC_T / 64; ++wv) d += __longlong_as_double((long long)s_p[wv][r][slot]);
      v = (unsigned long long)__double_as_longlong(d);
    }
    part[((b0 + r) * ntile + ct) * nslot + slot] = v;
  }
}

// one thread per (row, slot): the tiles in ascending order
__global__ __launch_bounds__(256) void concord_reduce_kernel(const unsigned long long* __restrict__ part, int64_t R, int ntile, int T,
                                                             int has_risk, int has_surv, long long* __restrict__ counts,
                                                             long long* __restrict__ rowcnt, double* __restrict__ sums) {
  const int nslot = cc_slots(T);
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= R * nslot) return;
  const int64_t r = id / nslot;
  const int slot = (int)(id - r * nslot);
  const unsigned long long* p = part + r * ntile * (int64_t)nslot + slot;
  if (slot < 5 + T) {
    unsigned long long v = 0;
    for (int c = 0; c < ntile; ++c) v += p[(int64_t)c * nslot];
    long long* cr = counts + r * 6;                      // [source][conc, tied, comp]
    if (slot == 0) { cr[2] = has_risk ? (long long)v : 0; cr[5] = has_surv ? (long long)v : 0; }
    else if (slot < 3) cr[slot - 1] = (long long)v;
    else if (slot < 5) cr[slot] = (long long)v;
    else rowcnt[r * (2 + T) + 2 + (slot - 5)] = (long long)v;
  } else {
    double v = 0.0;
    for (int c = 0; c < ntile; ++c) v += __longlong_as_double((long long)p[(int64_t)c * nslot]);
    const int q = (slot - 5 - T) / 5, s = (slot - 5 - T) - 5 * q;
    double* sr = sums + (r * 2 * T + q) * 3;             // source 0; source 1 lies 3 T further
    if (s == 0) { sr[2] = has_risk ? v : 0.0; sr[3 * T + 2] = has_surv ? v : 0.0; }
    else if (s < 3) sr[s - 1] = v;
    else sr[3 * T + s - 3] = v;
  }
}

static bool cc_shape_ok(int64_t n, int64_t R, int64_t T) {
  return n >= 1 && n <= (1 << 16) && R >= 1 && R <= (1 << 20) && T >= 1 && T <= CC_MAXT;
}

extern "C" size_t advmil_concord_rows_workspace_bytes(int64_t n, int R, int T) {
  if (!cc_shape_ok(n, R, T)) return 0;
  const size_t ntile = ((size_t)n + CC_T - 1) / CC_T;
  return (size_t)R * (size_t)n * sizeof(double) + (size_t)R * ntile * (size_t)cc_slots(T) * 8 + (((size_t)n + 1) & ~(size_t)1) * sizeof(int32_t);
}

extern "C" int advmil_concord_rows_plan(int* walk_rows, int* walk_trip, int* pair_tile, int* pair_rows) {
  if (!walk_rows || !walk_trip || !pair_tile || !pair_rows) return ADVMIL_EINVAL;
  *walk_rows = CC_WALK_ROWS; *walk_trip = 64; *pair_tile = CC_T; *pair_rows = CC_R;
  return ADVMIL_OK;
}

extern "C" int advmil_concord_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights,
                                   int64_t ldw, int R, const float* risk, const float* surv, int64_t lds, int Q, const int32_t* col,
                                   const float* tau, int T, int64_t* counts, int64_t* rowcnt, double* sums, void* ws, size_t ws_bytes,
                                   advmil_stream_t stream_) {
  if (!stime || !sevent || !order || !tau || !counts || !rowcnt || !sums || !ws) return ADVMIL_EINVAL;
  if (!risk && !surv) return ADVMIL_EINVAL;
  if (!cc_shape_ok(n, R, T)) return ADVMIL_EINVAL;
  if (weights && ldw < n) return ADVMIL_EINVAL;
  if (surv && (!col || Q < 1 || Q > 4096 || lds < Q)) return ADVMIL_EINVAL;
  if (((uintptr_t)stime & 3) || ((uintptr_t)sevent & 3) || ((uintptr_t)order & 3) || ((uintptr_t)weights & 3) || ((uintptr_t)risk & 3) ||
      ((uintptr_t)surv & 3) || ((uintptr_t)col & 3) || ((uintptr_t)tau & 3))
    return ADVMIL_EINVAL;
  if (((uintptr_t)counts & 7) || ((uintptr_t)rowcnt & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)ws & 7)) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_concord_rows_workspace_bytes(n, R, T)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int ni = (int)n, ntile = (ni + CC_T - 1) / CC_T, nslot = cc_slots(T);
  double* Gy = (double*)ws;                              // [R, n]: G at the block ends of the sorted order
  unsigned long long* part = (unsigned long long*)(Gy + (size_t)R * (size_t)n);       // [R, ntile, nslot]
  int32_t* bend = (int32_t*)(part + (size_t)R * (size_t)ntile * (size_t)nslot);
  hipLaunchKernelGGL(concord_prologue_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, stime, ni, bend);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(concord_walk_kernel, dim3((unsigned)((R + CC_WALK_ROWS - 1) / CC_WALK_ROWS)), dim3(64 * CC_WALK_ROWS), 0, stream, stime,
                     sevent, order, ni, weights, ldw, (int64_t)R, 2 + T, Gy, (long long*)rowcnt);
  ADVMIL_LAUNCH_CHECK();
  const dim3 grid((unsigned)((R + CC_R - 1) / CC_R), (unsigned)ntile);
#define CC_PAIRS(RK, SV)                                                                                                                  \
  hipLaunchKernelGGL((concord_pairs_kernel<RK, SV>), grid, dim3(CC_T), 0, stream, stime, sevent, order, ni, weights, ldw, (int64_t)R, risk, \
                     surv, lds, Q, col, tau, T, (const double*)Gy, (const int32_t*)bend, part)
  if (risk && surv) CC_PAIRS(true, true);
  else if (risk) CC_PAIRS(true, false);
  else CC_PAIRS(false, true);
#undef CC_PAIRS
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(concord_reduce_kernel, dim3((unsigned)(((int64_t)R * nslot + 255) / 256)), dim3(256), 0, stream,
                     (const unsigned long long*)part, (int64_t)R, ntile, T, risk ? 1 : 0, surv ? 1 : 0, (long long*)counts,
                     (long long*)rowcnt, sums);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
