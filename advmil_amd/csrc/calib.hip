// Censoring-aware time error and D-calibration of R rows (bootstrap resamples = integer weights) over ONE cohort: the hinge, margin and
// pseudo-observation absolute errors of up to 8 predicted-time columns, the event Kaplan-Meier curve's restricted mean, and the
// D-calibration bin masses (include/advmil_hip.h has the definitions). The cohort's sort by time and its tie blocks are the same for all
// rows; a block without weight in a row is a factor of exactly 1 and an interval over which the curve does not move, so every row walks
// the COHORT's blocks and keeps the row's own grid only in what it counts (K, u_K, the integral's end).
//
// The leave-one-out curve of a censored tie block k needs no pass over the other blocks. Lowering n_v by one for v <= k changes the
// factors at or before k only, and by the same amount whatever k is: with g_v = (n_v - 1 - d_v) / (n_v - 1), S'_v = prod_{x <= v} g_x
// and theta'_k = sum_{v <= k} S'_{v-1} (u_v - u_{v-1}) two more forward scans, and with the row's own factors f_v behind k,
//   theta^(-k) = theta'_k + S'_k T_k,   T_k = sum_{v > k} (prod_{k < x < v} f_x) (u_v - u_{v-1}) = A(u_k) / S(u_k),
// where T_k = (u_{k+1} - u_k) + f_{k+1} T_{k+1} is ONE backward scan of affine maps -- and the margin surrogate's A / S without the
// division. So a row costs O(n) with the pseudo-observation as without it; the K^2 form is never needed.
//
// Launches on the caller's stream:
//   walk   one wavefront per row, CB_WALK_ROWS rows per workgroup, 64 sorted samples per trip, three sweeps:
//          1 the row's total weight; 2 ascending: the integer scans of concord.hip's walk give every block's n and d, product and sum
//          scans give S, theta, S', theta' at every block end (into the workspace) and the NEXT block's (f, du) is left at this block's
//          end; 3 descending: the backward scan of the maps y -> du + f y gives every sample its block's T, the block-end values are
//          broadcast to the block's samples (a block may straddle trips: carried), and each lane adds its sample's terms to its own
//          double accumulators; one fixed butterfly per sum at the end, lane 0 writes every slot;
//   dcal   (only with p_own) one wavefront per row: each lane owns a column of 2 B double slots in LDS (the mass a sample adds to its
//          own bin, and the mass it adds to EVERY bin below: the prefix form), so no two lanes ever touch a slot; a butterfly per slot
//          and a suffix sum over the bins end the row.
// No atomics anywhere; which lane adds which term in which order depends on n and the lane only, never on R or on the row's place in
// the batch: a row of a batch has the bits of the one-row call, run after run.
#include "common.h"
#include "../../include/advmil_hip.h"

constexpr int CB_WALK_ROWS = 4;                          // rows (wavefronts) per workgroup of the walk
constexpr int CB_MAXP = 8;                               // prediction columns
constexpr int CB_MAXB = 32;                              // D-calibration bins

__device__ __forceinline__ uint32_t cb_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t cb_scan_add(uint32_t v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}
__device__ __forceinline__ double cb_scan_add(double v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}
__device__ __forceinline__ double cb_scan_mul(double v, int lane) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double u = __shfl_up(v, s, 64);
    if (lane >= s) v *= u;
  }
  return v;
}

__global__ __launch_bounds__(64 * CB_WALK_ROWS) void calib_walk_kernel(const float* __restrict__ stime, const float* __restrict__ sevent,
                                                                       const int32_t* __restrict__ order, int n,
                                                                       const int32_t* __restrict__ weights, int64_t ldw, int64_t R,
                                                                       const float* __restrict__ pred, int64_t ldp, int P, float gamma_,
                                                                       int with_po, int nws, double* __restrict__ wsd,
                                                                       long long* __restrict__ rowcnt, double* __restrict__ km,
                                                                       double* __restrict__ err, double* __restrict__ dcal_zero, int B) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * CB_WALK_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;                                    // (a whole wave: nothing below crosses waves)
  const int32_t* w = weights ? weights + r * ldw : nullptr;
  double* Sx = wsd + r * (int64_t)nws * n;               // S at the block ends
  double* Fn = Sx + n;                                   // at a block end: the NEXT block's factor ...
  double* An = Fn + n;                                   // ... and interval (0 behind the row's largest time)
  double* Spx = An + n;                                  // with_po only: S' and theta' at the block ends
  double* Thp = Spx + n;
  const double gamma = (double)gamma_;

  // ---- sweep 1: the total the at-risk counts start from ----
  uint32_t tw = 0;
  for (int k = lane; k < n; k += 64) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint32_t)n) o = 0;                         // a permutation is the caller's duty; no address outside a row in any case
    tw += w ? (uint32_t)w[o] : 1u;
  }
  tw = cb_wave_sum(tw);

  // ---- sweep 2: ascending over the tie blocks ----
  uint32_t cw = 0, ce = 0;                               // the two sums through the previous trip ...
  uint32_t bw = 0, be = 0;                               // ... and at the last block end so far
  double bt = 0.0;                                       // the last block end's time (u_0 = 0) ...
  int pend = -1;                                         // ... and its place
  double PS = 1.0, PP = 1.0, TH = 0.0, THP = 0.0;        // running S, S', theta, theta'
  double uK = 0.0;                                       // the largest time with weight
  uint32_t K = 0;                                        // blocks with weight
#pragma unroll 1
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool in = k < n;
    bool end = false, ek = false;
    uint32_t wk = 0;
    double tk = 0.0;
    if (in) {
      const float tf = stime[k];
      tk = (double)tf;
      end = (k + 1 == n) || (stime[k + 1] != tf);
      uint32_t o = (uint32_t)order[k];
      if (o >= (uint32_t)n) o = 0;
      wk = w ? (uint32_t)w[o] : 1u;
      ek = sevent[k] != 0.0f;
    }
    const uint32_t pw = cw + cb_scan_add(wk, lane), pe = ce + cb_scan_add(ek ? wk : 0u, lane);
    const unsigned long long ends = __ballot(end);
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : lane;
    uint32_t qw = __shfl(pw, pl, 64), qe = __shfl(pe, pl, 64);
    double tprev = __shfl(tk, pl, 64);
    int iprev = base + pl;
    if (!below) { qw = bw; qe = be; tprev = bt; iprev = pend; }
    double f = 1.0, g = 1.0, a = 0.0;
    bool pos = false;
    if (end) {
      const uint32_t nn = tw - qw, d = pe - qe;          // at risk and events of the block
      pos = pw != qw;
      if (d) {
        f = (double)(nn - d) / (double)nn;
        if (nn - 1u >= d) g = (double)(nn - 1u - d) / (double)(nn - 1u);    // (d > 0: nn - 1 >= d > 0; not so only behind the last censoring)
      }
      if (nn) a = tk - tprev;                            // nobody at risk: behind the row's largest time
    }
    const double sS = PS * cb_scan_mul(f, lane), sP = PP * cb_scan_mul(g, lane);
    double sprev = __shfl_up(sS, 1, 64), pprev = __shfl_up(sP, 1, 64);
    if (lane == 0) { sprev = PS; pprev = PP; }
    const double th = TH + cb_scan_add(a * sprev, lane), thp = THP + cb_scan_add(a * pprev, lane);
    if (end) {
      Sx[k] = sS;
      if (with_po) { Spx[k] = sP; Thp[k] = thp; }
      if (iprev >= 0) { Fn[iprev] = f; An[iprev] = a; }
    }
    cw = __shfl(pw, 63, 64); ce = __shfl(pe, 63, 64);
    if (ends) {
      const int hl = 63 - __clzll((long long)ends);
      bw = __shfl(pw, hl, 64); be = __shfl(pe, hl, 64); bt = __shfl(tk, hl, 64);
      pend = base + hl;
    }
    const unsigned long long posm = __ballot(end && pos);
    if (posm) {
      K += (uint32_t)__popcll(posm);
      uK = __shfl(tk, 63 - __clzll((long long)posm), 64);
    }
    PS = __shfl(sS, 63, 64); PP = __shfl(sP, 63, 64); TH = __shfl(th, 63, 64); THP = __shfl(thp, 63, 64);
  }
  const double N = (double)tw, theta = TH;
  __threadfence_block();                                 // sweep 3 reads Fn / An where ANOTHER lane of this wave left them

  // ---- sweep 3: descending; T of every block, and the samples' terms ----
  double num[CB_MAXP][3];
#pragma unroll
  for (int c = 0; c < CB_MAXP; ++c) { num[c][0] = 0.0; num[c][1] = 0.0; num[c][2] = 0.0; }
  double den = 0.0;                                      // sum w omega
  uint32_t z0 = 0;                                       // weight of the censored samples with S = 0
  double Zin = 0.0;                                      // T of the block that holds the first sample of the trip above
  double cS = 1.0, cSp = 1.0, cThp = 0.0;                // the block-end values of the lowest block end above
#pragma unroll 1
  for (int base = ((n - 1) >> 6) << 6; base >= 0; base -= 64) {
    const int k = base + lane;
    const bool in = k < n;
    bool end = false, ek = false;
    uint32_t wk = 0, o = 0;
    double tk = 0.0;
    if (in) {
      const float tf = stime[k];
      tk = (double)tf;
      end = (k + 1 == n) || (stime[k + 1] != tf);
      o = (uint32_t)order[k];
      if (o >= (uint32_t)n) o = 0;
      wk = w ? (uint32_t)w[o] : 1u;
      ek = sevent[k] != 0.0f;
    }
    double M = 1.0, C = 0.0;                             // this place's map y -> C + M y (the identity inside a block and at the last end)
    double sv = 1.0, spv = 1.0, thpv = 0.0;
    if (end) {
      if (k + 1 < n) { M = Fn[k]; C = An[k]; }
      sv = Sx[k];
      if (with_po) { spv = Spx[k]; thpv = Thp[k]; }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {                   // the maps of the places lane ... 63, composed
      const double M2 = __shfl_down(M, s, 64), C2 = __shfl_down(C, s, 64);
      if (lane + s < 64) { C = C + M * C2; M = M * M2; }
    }
    const double T = C + M * Zin;                        // T of the block this place lies in
    const unsigned long long ends = __ballot(end);
    const unsigned long long above = ends & (~0ull << lane);
    const int el = above ? __ffsll((long long)above) - 1 : lane;
    double bS = __shfl(sv, el, 64), bSp = __shfl(spv, el, 64), bThp = __shfl(thpv, el, 64);
    if (!above) { bS = cS; bSp = cSp; bThp = cThp; }
    if (ends) {
      const int lo = __ffsll((long long)ends) - 1;
      cS = __shfl(sv, lo, 64); cSp = __shfl(spv, lo, 64); cThp = __shfl(thpv, lo, 64);
    }
    Zin = __shfl(T, 0, 64);
    if (in && wk) {
      const double wd = (double)wk;
      double omega = 1.0, m = tk, s = tk;
      if (!ek) {
        omega = 1.0 - bS;
        if (bS > 0.0) m = tk + T; else z0 += wk;
        s = N * theta - (N - 1.0) * (bThp + bSp * T);
      }
      const double wo = wd * omega;
      den += wo;
      if (pred) {
        const float* pr = pred + (int64_t)o * ldp;
#pragma unroll
        for (int c = 0; c < CB_MAXP; ++c) {
          if (c < P) {
            const double y = (double)pr[c];
            const double h = ek ? fabs(tk - y) : fmax(0.0, tk + gamma - y);
            num[c][0] += wd * h;
            num[c][1] += wo * fabs(m - y);
            if (with_po) num[c][2] += wo * fabs(s - y);
          }
        }
      }
    }
  }
  den = cb_wave_sum(den);
  z0 = cb_wave_sum(z0);
#pragma unroll
  for (int c = 0; c < CB_MAXP; ++c) {
    if (c < P) {
      const double h = cb_wave_sum(num[c][0]), mg = cb_wave_sum(num[c][1]), po = cb_wave_sum(num[c][2]);
      if (lane == 0) {
        double* e = err + (r * P + c) * 6;
        const bool has = pred != nullptr;
        e[0] = has ? h : 0.0;  e[1] = has ? N : 0.0;
        e[2] = has ? mg : 0.0; e[3] = has ? den : 0.0;
        e[4] = has && with_po ? po : 0.0; e[5] = has && with_po ? den : 0.0;
      }
    }
  }
  if (lane == 0) {
    rowcnt[r * 4] = tw; rowcnt[r * 4 + 1] = ce; rowcnt[r * 4 + 2] = K; rowcnt[r * 4 + 3] = z0;
    km[r * 3] = theta; km[r * 3 + 1] = PS; km[r * 3 + 2] = uK;
  }
  if (dcal_zero && lane < B) dcal_zero[r * B + lane] = 0.0;      // no p_own: the masses are written as 0
}

__global__ __launch_bounds__(64) void calib_dcal_kernel(const float* __restrict__ sevent, const int32_t* __restrict__ order, int n,
                                                        const int32_t* __restrict__ weights, int64_t ldw,
                                                        const float* __restrict__ p_own, int B, double* __restrict__ dcal) {
  __shared__ double acc[2 * CB_MAXB][64];                // [slot][lane]: a lane's column; slots 0 .. B-1 own bin, B .. 2B-1 every bin below
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int32_t* w = weights ? weights + r * ldw : nullptr;
  for (int j = 0; j < 2 * B; ++j) acc[j][lane] = 0.0;
  const float Bf = (float)B;
  const double Bd = (double)B;
  for (int k = lane; k < n; k += 64) {
    uint32_t o = (uint32_t)order[k];
    if (o >= (uint32_t)n) o = 0;
    const uint32_t wk = w ? (uint32_t)w[o] : 1u;
    if (!wk) continue;
    const float p = p_own[o];
    int kb = (int)(p * Bf);
    kb = kb < B - 1 ? kb : B - 1;
    kb = kb > 0 ? kb : 0;                                // p in [0, 1] is the caller's duty; no slot outside the column in any case
    const double wd = (double)wk, pd = (double)p;
    if (sevent[k] != 0.0f || !(p > 0.0f)) {
      acc[sevent[k] != 0.0f ? kb : 0][lane] += wd;
    } else {
      acc[kb][lane] += wd * (pd - (double)kb / Bd) / pd;
      acc[B + kb][lane] += wd / (Bd * pd);
    }
  }
  double mine = 0.0;                                     // lane j < B: the own-bin sum of bin j; lane B + j: what bin j hands to every bin below
  for (int j = 0; j < 2 * B; ++j) {
    const double v = cb_wave_sum(acc[j][lane]);
    if (lane == j) mine = v;
  }
  double run = 0.0;
  for (int j = B - 1; j >= 0; --j) {
    const double own = __shfl(mine, j, 64), down = __shfl(mine, B + j, 64);
    if (lane == 0) dcal[r * B + j] = own + run;
    run += down;
  }
}

static bool cb_shape_ok(int64_t n, int64_t R) { return n >= 1 && n <= (1 << 16) && R >= 1 && R <= (1 << 20); }

extern "C" size_t advmil_calib_rows_workspace_bytes(int64_t n, int R, int with_po) {
  if (!cb_shape_ok(n, R) || (with_po != 0 && with_po != 1)) return 0;
  return (size_t)R * (size_t)n * (size_t)(3 + 2 * with_po) * sizeof(double);
}

extern "C" int advmil_calib_rows_plan(int* walk_rows, int* walk_trip, int* dcal_rows) {
  if (!walk_rows || !walk_trip || !dcal_rows) return ADVMIL_EINVAL;
  *walk_rows = CB_WALK_ROWS; *walk_trip = 64; *dcal_rows = 1;
  return ADVMIL_OK;
}

extern "C" int advmil_calib_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights,
                                 int64_t ldw, int R, const float* pred, int64_t ldp, int P, const float* p_own, int bins, float gamma,
                                 int with_po, int64_t* rowcnt, double* km, double* err, double* dcal, void* ws, size_t ws_bytes,
                                 advmil_stream_t stream_) {
  if (!stime || !sevent || !order || !rowcnt || !km || !err || !dcal || !ws) return ADVMIL_EINVAL;
  if (!pred && !p_own) return ADVMIL_EINVAL;
  if (!cb_shape_ok(n, R) || P < 1 || P > CB_MAXP || bins < 2 || bins > CB_MAXB) return ADVMIL_EINVAL;
  if ((with_po != 0 && with_po != 1) || !(gamma == gamma)) return ADVMIL_EINVAL;
  if (weights && ldw < n) return ADVMIL_EINVAL;
  if (pred && ldp < P) return ADVMIL_EINVAL;
  if (((uintptr_t)stime & 3) || ((uintptr_t)sevent & 3) || ((uintptr_t)order & 3) || ((uintptr_t)weights & 3) || ((uintptr_t)pred & 3) ||
      ((uintptr_t)p_own & 3))
    return ADVMIL_EINVAL;
  if (((uintptr_t)rowcnt & 7) || ((uintptr_t)km & 7) || ((uintptr_t)err & 7) || ((uintptr_t)dcal & 7) || ((uintptr_t)ws & 7))
    return ADVMIL_EINVAL;
  if (ws_bytes < advmil_calib_rows_workspace_bytes(n, R, with_po)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(calib_walk_kernel, dim3((unsigned)((R + CB_WALK_ROWS - 1) / CB_WALK_ROWS)), dim3(64 * CB_WALK_ROWS), 0, stream, stime,
                     sevent, order, (int)n, weights, ldw, (int64_t)R, pred, ldp, P, gamma, with_po, 3 + 2 * with_po, (double*)ws,
                     (long long*)rowcnt, km, err, p_own ? (double*)nullptr : dcal, bins);
  ADVMIL_LAUNCH_CHECK();
  if (p_own) {
    hipLaunchKernelGGL(calib_dcal_kernel, dim3((unsigned)R), dim3(64), 0, stream, sevent, order, (int)n, weights, ldw, p_own, bins, dcal);
    ADVMIL_LAUNCH_CHECK();
  }
  return ADVMIL_OK;
}
