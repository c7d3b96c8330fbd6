// Survival evaluators and the ranking loss (reference eval/evaluator.py, loss/utils.py:43-80, 123-133, 155-175): the per-epoch
// evaluation of a collector as one or two launches per family instead of ten to twelve host computations, and the two O(n^2) pair
// losses (rank_loss, SurvPLE) in the shape of cindex_counts_kernel: a workgroup per anchor sample, 256 threads over the partners.
//
// Arithmetic, stated plainly: every per-element / per-pair term is formed in fp32, as the reference forms it. exp and log of a term
// go through the hw_* wrappers of common.h (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp). Every SUM is carried in double from the first
// addition on. The few per-anchor / final transcendentals (the log of a risk-set sum, the rescaling exp of the softmax merge) are
// double-precision libm. No floating-point atomics anywhere: per-workgroup partials go to the caller's workspace and a second
// launch merges them in a fixed order, so a result does not depend on the launch's scheduling or on what the buffers held before.
#include "common.h"
#include "../../include/advmil_hip.h"

namespace {

constexpr int kMaxBlocks = 1024;        // grid of the O(n) passes (grid-stride beyond it)
constexpr int kSlots = 16;              // doubles per workgroup partial / per result array of the O(n) passes

inline int linear_blocks(int64_t n) { return (int)((n + 255) / 256 < kMaxBlocks ? (n + 255) / 256 : kMaxBlocks); }

// fixed-order sum over the workgroup: [q][256] doubles in LDS, halving tree; the result is in red[q][0] after the last barrier
template <int Q>
__device__ __forceinline__ void block_tree_sum(double (&red)[Q][256]) {
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int q = 0; q < Q; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
}

// the discriminator's fake-only term (loss/utils.py:182-203 with real = None): which 0 = bce as shipped, 1 = hinge, 2 = wasserstein
__device__ __forceinline__ float fake_term(int which, float f) {
  const float sg = hw_rcp(1.0f + hw_exp(-f));
  const float t_bce = -(1.0f - hw_log(sg + 1e-8f));
  const float t_hin = fmaxf(1.0f + f, 0.0f);
  return which == 0 ? t_bce : (which == 1 ? t_hin : f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ContSurv_Evaluator: every O(n) quantity in one pass. Partial p of workgroup b: ws[b * kSlots + q].
//  0 sum recon terms at alpha   1 ... at alpha = 0   2 sum `mae` terms (recon_loss defaults: gamma 1, l1, alpha 0)
//  3 sum fake-only discriminator terms   4 sum fake
//  5 sum_{e==1} |t - p|   6 sum_{e==0} relu(t - p)   7 sum_{e==1} (p - t)   8 sum_{e==0} -relu(t - p)      (RAE / NRE numerators)
//  9 #(e == 1)   10 #(e == 0)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surv_cont_partial_kernel(const float* __restrict__ t, const float* __restrict__ e,
                                                                const float* __restrict__ pred, const float* __restrict__ fake,
                                                                int64_t n, float alpha, float gamma, int l2, int which,
                                                                double* __restrict__ ws) {
  double acc[11];
#pragma unroll
  for (int q = 0; q < 11; ++q) acc[q] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float ti = t[i], ei = e[i], p = pred[i];
    const float d = p - ti;
    float obs = ei * fabsf(d), cen = (1.0f - ei) * fmaxf(gamma - d, 0.0f);
    if (l2) { obs *= obs; cen *= cen; }
    const float rec = obs + cen;
    acc[0] += (double)((1.0f - alpha) * rec + alpha * obs);
    acc[1] += (double)rec;
    acc[2] += (double)(ei * fabsf(d) + (1.0f - ei) * fmaxf(1.0f - d, 0.0f));
    if (fake) {
      const float f = fake[i];
      acc[3] += (double)fake_term(which, f);
      acc[4] += (double)f;
    }
    if (ei == 1.0f) {
      acc[5] += (double)fabsf(ti - p);
      acc[7] += (double)d;
      acc[9] += 1.0;
    }
    if (ei == 0.0f) {
      const float r = fmaxf(ti - p, 0.0f);
      acc[6] += (double)r;
      acc[8] -= (double)r;
      acc[10] += 1.0;
    }
  }
  __shared__ double red[11][256];
#pragma unroll
  for (int q = 0; q < 11; ++q) red[q][threadIdx.x] = acc[q];
  block_tree_sum<11>(red);
  if (threadIdx.x < kSlots) ws[(int64_t)blockIdx.x * kSlots + threadIdx.x] = threadIdx.x < 11 ? red[threadIdx.x][0] : 0.0;
}

// Merge of `blocks` partials of kSlots doubles, one workgroup: thread (g, q) = (tid / 16, tid % 16) adds the partials g, g + 16, ... of
// slot q in ascending order, thread q adds the 16 group sums in ascending order. scale[q] multiplies slot q (RAE / NRE: 1 / end_time).
__global__ __launch_bounds__(256) void surv_merge_kernel(const double* __restrict__ ws, int blocks, double s5678,
                                                         double* __restrict__ out) {
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  double a = 0.0;
  for (int b = g; b < blocks; b += 16) a += ws[(int64_t)b * kSlots + q];
  __shared__ double part[16][16];
  part[g][q] = a;
  __syncthreads();
  if (threadIdx.x < kSlots) {
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) r += part[k][threadIdx.x];
    if (threadIdx.x >= 5 && threadIdx.x <= 8) r *= s5678;
    out[threadIdx.x] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// DiscSurv_Evaluator: a thread per row. S_k = prod_{l<=k} (1 - h_l) as a running fp32 product (torch.cumprod), risk = sum_k S_k.
// The bin index selects by COMPARISON inside the walk over the row (k == bin), never as an address; a row whose index is outside
// [0, bins - 1] (or not a number) contributes nothing and is counted in slot 4.
//  0 sum SurvMLE terms at alpha   1 ... at alpha = 0   2 sum fake-only discriminator terms   3 sum fake   4 #rows with a bad bin index
//
// The risk is the reference's float32 number BIT FOR BIT: it goes, negated, into the concordance index, where a pair is a tie only
// within 1e-8, so a last-bit difference moves pairs between "tied" and "ordered" whenever two rows hold the same hazards in another
// order (quantised or saturating hazards). The reference forms it as np.sum(np.cumprod(1 - h, axis=1), axis=1) in float32, hence
//  - 1 - h, the running product and every addition are single rounded operations (no contraction into v_fma / v_fmac);
//  - the additions follow numpy's pairwise sum over a contiguous row: fewer than 8 elements in order; up to 128 elements eight
//    accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... < n - n % 8, then ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the
//    last n % 8 elements in order; above 128 a split at n2 = n / 2 - (n / 2) % 8, both halves by the same rule, left + right.
// For bins <= 256 that is at most three leaves, A | B or A | (B1 | B2), walked in one pass over the row.
// ---------------------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
struct DiscRowWalk {                                            // the running product over one row and what SurvMLE gathers from it
  const float* row;
  int bin, k;
  float S, S_prev, S_at, h_at;
  __host__ __device__ __forceinline__ float next() {            // -> S_k, and steps to k + 1
    const float h = row[k];
    const float om = 1.0f - h;
    const float Sn = S * om;
    if (k == bin) { S_prev = S; S_at = Sn; h_at = h; }
    S = Sn;
    ++k;
    return Sn;
  }
};

// numpy's pairwise leaf (len <= 128) over the next `len` elements of the walk
__host__ __device__ __forceinline__ float np_leaf_sum(DiscRowWalk& w, int len) {
  if (len < 8) {
    float res = 0.0f;
    for (int i = 0; i < len; ++i) res = res + w.next();
    return res;
  }
  float r0 = w.next(), r1 = w.next(), r2 = w.next(), r3 = w.next(), r4 = w.next(), r5 = w.next(), r6 = w.next(), r7 = w.next();
  const int body = len - len % 8;
  for (int i = 8; i < body; i += 8) {
    r0 = r0 + w.next(); r1 = r1 + w.next(); r2 = r2 + w.next(); r3 = r3 + w.next();
    r4 = r4 + w.next(); r5 = r5 + w.next(); r6 = r6 + w.next(); r7 = r7 + w.next();
  }
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = body; i < len; ++i) res = res + w.next();
  return res;
}

// np.sum over the `n` <= 256 elements of the walk
__host__ __device__ __forceinline__ float np_row_sum(DiscRowWalk& w, int n) {
  if (n <= 128) return np_leaf_sum(w, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  const float left = np_leaf_sum(w, n2);
  const int nr = n - n2;                                        // <= 135
  if (nr <= 128) return left + np_leaf_sum(w, nr);
  int m = nr / 2;
  m -= m % 8;
  const float b1 = np_leaf_sum(w, m);
  const float b2 = np_leaf_sum(w, nr - m);
  return left + (b1 + b2);
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(256) void surv_disc_partial_kernel(const float* __restrict__ hz, int64_t ld, const float* __restrict__ t,
                                                                const float* __restrict__ e, const float* __restrict__ fake,
                                                                int64_t n, int bins, float alpha, float eps, int which,
                                                                float* __restrict__ risk, double* __restrict__ ws) {
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float tf = truncf(t[i]);                        // .long() of the reference truncates toward zero
    const bool ok = tf >= 0.0f && tf <= (float)(bins - 1);
    const int bin = ok ? (int)tf : -1;
    DiscRowWalk w{hz + i * ld, bin, 0, 1.0f, 1.0f, 1.0f, 1.0f};
    risk[i] = np_row_sum(w, bins);
    const float S_prev = w.S_prev, S_at = w.S_at, h_at = w.h_at;
    if (ok) {
      const float ei = e[i], c = 1.0f - ei;
      const float unc = -(1.0f - c) * (hw_log(fmaxf(S_prev, eps)) + hw_log(fmaxf(h_at, eps)));
      const float cen = -c * hw_log(fmaxf(S_at, eps));
      const float neg = cen + unc;
      acc[0] += (double)((1.0f - alpha) * neg + alpha * unc);
      acc[1] += (double)neg;
    } else {
      acc[4] += 1.0;
    }
    if (fake) {
      const float f = fake[i];
      acc[2] += (double)fake_term(which, f);
      acc[3] += (double)f;
    }
  }
  __shared__ double red[5][256];
#pragma unroll
  for (int q = 0; q < 5; ++q) red[q][threadIdx.x] = acc[q];
  block_tree_sum<5>(red);
  if (threadIdx.x < kSlots) ws[(int64_t)blockIdx.x * kSlots + threadIdx.x] = threadIdx.x < 5 ? red[threadIdx.x][0] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// SurvPLE: workgroup i forms sum_j [T_j >= T_i] exp(min(theta_j, 10)) (fp32 exp, double sum) and leaves
// term_i = (theta_i - log(sum)) * E_i (double log) in ws[i]; the merge writes out[0] = -sum_i term_i / n, out[1] = sum_i E_i.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ple_terms_kernel(const float* __restrict__ theta, const float* __restrict__ T,
                                                        const float* __restrict__ E, int64_t n, double* __restrict__ ws) {
  const int64_t i = blockIdx.x;
  const float Ti = T[i];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += 256)
    if (T[j] >= Ti) s += (double)hw_exp(fminf(theta[j], 10.0f));
  __shared__ double red[1][256];
  red[0][threadIdx.x] = s;
  block_tree_sum<1>(red);
  if (threadIdx.x == 0) {
    const float th = theta[i];
    const double thc = (double)(th > 10.0f ? 10.0f : th);        // torch.where(y_hat > 10, 10, y_hat): a NaN stays a NaN
    ws[i] = (thc - log(red[0][0])) * (double)E[i];
    ws[n + i] = (double)E[i];
  }
}

// One workgroup: fixed-order sums of the arrays ws[0..n) and ws[n..2n) -> out[0] = -a / n, out[1] = b.
__global__ __launch_bounds__(256) void ple_merge_kernel(const double* __restrict__ ws, int64_t n, double* __restrict__ out) {
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) { a += ws[i]; b += ws[n + i]; }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
  block_tree_sum<2>(red);
  if (threadIdx.x == 0) { out[0] = -red[0][0] / (double)n; out[1] = red[1][0]; }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rank_loss (loss/utils.py:43-80). Pairs (i, j) with e_i == 1 and t_i < t_j; x_ij = p_i - p_j; L_ij = relu(gamma + x_ij), squared for l2.
// Uniform weights:  loss = sum L / P,  P = number of pairs.
// add_weight:       loss = sum exp(x - M) L / Z,  Z = sum exp(x - M),  M = max x over the pairs (the reference's `maxx` is M plus a
//                   constant ~1e-5, which cancels between numerator and denominator).
// Workgroup i leaves in ws (four arrays of n doubles): s_i = sum_j w L, z_i = sum_j w (w = 1 or exp(x - m_i)), m_i = max_j x (its
// own maximum, -inf without a pair) and c_i = its pair count (int64). The merge rescales by exp(m_i - M) in double.
// state[0..3] = loss, P or Z, M, P (as double; 0 = no pair: loss 0).
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rank_pair_loss(float v, int l2) {       // v = gamma + x
  const float r = fmaxf(v, 0.0f);
  return l2 ? r * r : r;
}

__global__ __launch_bounds__(256) void rank_fwd_anchor_kernel(const float* __restrict__ pred, const float* __restrict__ t,
                                                              const float* __restrict__ e, int64_t n, float gamma, int l2,
                                                              int add_weight, double* __restrict__ ws) {
  const int64_t i = blockIdx.x;
  double* ws_s = ws;
  double* ws_z = ws + n;
  double* ws_m = ws + 2 * n;
  long long* ws_c = (long long*)(ws + 3 * n);
  const double ninf = -__builtin_huge_val();
  if (!(e[i] == 1.0f)) {                                         // not an anchor: neutral partials (every slot is written)
    if (threadIdx.x == 0) { ws_s[i] = 0.0; ws_z[i] = 0.0; ws_m[i] = ninf; ws_c[i] = 0; }
    return;
  }
  const float ti = t[i], pi = pred[i];
  __shared__ double red[2][256];
  __shared__ float fmin_s[4];
  float mi = 0.0f;                                               // m_i = p_i - min_j p_j over the partners
  if (add_weight) {
    float pmin = __builtin_huge_valf();
    for (int64_t j = threadIdx.x; j < n; j += 256)
      if (ti < t[j]) pmin = fminf(pmin, pred[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pmin = fminf(pmin, __shfl_xor(pmin, o, 64));
    if ((threadIdx.x & 63) == 0) fmin_s[threadIdx.x >> 6] = pmin;
    __syncthreads();
    pmin = fminf(fminf(fmin_s[0], fmin_s[1]), fminf(fmin_s[2], fmin_s[3]));
    mi = pi - pmin;                                              // -inf when there is no partner: no pair term is formed below
  }
  double s = 0.0, z = 0.0;
  long long c = 0;
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    if (!(ti < t[j])) continue;
    const float x = pi - pred[j];
    const float L = rank_pair_loss(gamma + x, l2);
    ++c;
    if (add_weight) {
      const float w = hw_exp(x - mi);
      s += (double)(w * L);
      z += (double)w;
    } else {
      s += (double)L;
    }
  }
  red[0][threadIdx.x] = s; red[1][threadIdx.x] = z;
  __shared__ long long cred[256];
  cred[threadIdx.x] = c;
  block_tree_sum<2>(red);
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) cred[threadIdx.x] += cred[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long cnt = cred[0];
    ws_s[i] = red[0][0];
    ws_z[i] = add_weight ? red[1][0] : (double)cnt;
    ws_m[i] = (add_weight && cnt > 0) ? (double)mi : ninf;
    ws_c[i] = cnt;
  }
}

__global__ __launch_bounds__(256) void rank_fwd_merge_kernel(const double* __restrict__ ws, int64_t n, int add_weight,
                                                             double* __restrict__ state, float* __restrict__ loss) {
  const double* ws_s = ws;
  const double* ws_z = ws + n;
  const double* ws_m = ws + 2 * n;
  const long long* ws_c = (const long long*)(ws + 3 * n);
  const double ninf = -__builtin_huge_val();
  __shared__ double red[2][256];
  __shared__ long long cred[256];
  double M = ninf;
  if (add_weight) {
    for (int64_t i = threadIdx.x; i < n; i += 256) M = fmax(M, ws_m[i]);
    red[0][threadIdx.x] = M;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[0][threadIdx.x] = fmax(red[0][threadIdx.x], red[0][threadIdx.x + st]);
      __syncthreads();
    }
    M = red[0][0];
    __syncthreads();
  }
  double s = 0.0, z = 0.0;
  long long c = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const long long ci = ws_c[i];
    if (ci == 0) continue;
    const double r = add_weight ? exp(ws_m[i] - M) : 1.0;
    s += r * ws_s[i];
    z += r * ws_z[i];
    c += ci;
  }
  red[0][threadIdx.x] = s; red[1][threadIdx.x] = z; cred[threadIdx.x] = c;
  block_tree_sum<2>(red);
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) cred[threadIdx.x] += cred[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long P = cred[0];
    const double l = P > 0 ? red[0][0] / red[1][0] : 0.0;
    state[0] = l;
    state[1] = P > 0 ? red[1][0] : 0.0;
    state[2] = (P > 0 && add_weight) ? M : 0.0;
    state[3] = (double)P;
    loss[0] = (float)l;
  }
}

// d loss / d x_ij = w_ij L'_ij (uniform, w = 1 / P) or w_ij (L'_ij + L_ij - loss) (softmax weights, w = exp(x - M) / Z);
// dp_k = gout * (sum_j dx_kj - sum_i dx_ik). Workgroup k walks all partners once and takes both roles.
__global__ __launch_bounds__(256) void rank_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ t,
                                                       const float* __restrict__ e, int64_t n, float gamma, int l2, int add_weight,
                                                       const double* __restrict__ state, const float* __restrict__ gout,
                                                       float* __restrict__ dpred) {
  const int64_t k = blockIdx.x;
  const double P = state[3];
  if (!(P > 0.0)) {                                              // no pair at all: gradient 0, written here
    if (threadIdx.x == 0) dpred[k] = 0.0f;
    return;
  }
  const float loss = (float)state[0], M = (float)state[2];
  const float tk = t[k], pk = pred[k];
  const bool anchor_k = e[k] == 1.0f;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    const float tj = t[j];
    const bool out_pair = anchor_k && tk < tj;                   // (k, j)
    const bool in_pair = tj < tk && e[j] == 1.0f;                // (j, k)
    if (!(out_pair || in_pair)) continue;                        // at most one of the two holds
    const float x = out_pair ? pk - pred[j] : pred[j] - pk;
    const float v = gamma + x;
    const float dL = l2 ? 2.0f * fmaxf(v, 0.0f) : (v > 0.0f ? 1.0f : 0.0f);
    float d;
    if (add_weight) d = hw_exp(x - M) * (dL + rank_pair_loss(v, l2) - loss);
    else d = dL;
    acc += out_pair ? (double)d : -(double)d;
  }
  __shared__ double red[1][256];
  red[0][threadIdx.x] = acc;
  block_tree_sum<1>(red);
  if (threadIdx.x == 0) dpred[k] = (float)(red[0][0] / state[1] * (double)gout[0]);
}

}  // namespace

extern "C" size_t advmil_surv_metrics_cont_workspace_bytes(int64_t n) {
  return n > 0 ? (size_t)linear_blocks(n) * kSlots * sizeof(double) : 0;
}
extern "C" size_t advmil_surv_metrics_disc_workspace_bytes(int64_t n) {
  return n > 0 ? (size_t)linear_blocks(n) * kSlots * sizeof(double) : 0;
}
extern "C" size_t advmil_ple_loss_workspace_bytes(int64_t n) { return n > 0 ? (size_t)n * 2 * sizeof(double) : 0; }
extern "C" size_t advmil_rank_loss_workspace_bytes(int64_t n) { return n > 0 ? (size_t)n * 4 * sizeof(double) : 0; }

extern "C" int advmil_surv_metrics_cont(const float* t, const float* e, const float* pred, const float* fake, int64_t n, float alpha,
                                        float gamma, int l2, float end_time, int which, double* out16, void* ws, size_t ws_bytes,
                                        advmil_stream_t stream_) {
  if (!t || !e || !pred || !out16 || !ws || n <= 0 || n > 0x7fffffff || which < 0 || which > 2 || !(end_time != 0.0f))
    return ADVMIL_EINVAL;
  if (ws_bytes < advmil_surv_metrics_cont_workspace_bytes(n)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = linear_blocks(n);
  hipLaunchKernelGGL(surv_cont_partial_kernel, dim3(blocks), dim3(256), 0, stream, t, e, pred, fake, n, alpha, gamma, l2, which,
                     (double*)ws);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(surv_merge_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, blocks, 1.0 / (double)end_time, out16);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_surv_metrics_disc(const float* hazards, int64_t ld, const float* t, const float* e, const float* fake, int64_t n,
                                        int bins, float alpha, float eps, int which, float* risk, double* out16, void* ws,
                                        size_t ws_bytes, advmil_stream_t stream_) {
  if (!hazards || !t || !e || !risk || !out16 || !ws || n <= 0 || n > 0x7fffffff || bins < 1 || bins > 256 || ld < bins || which < 0 ||
      which > 2)
    return ADVMIL_EINVAL;
  if (ws_bytes < advmil_surv_metrics_disc_workspace_bytes(n)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = linear_blocks(n);
  hipLaunchKernelGGL(surv_disc_partial_kernel, dim3(blocks), dim3(256), 0, stream, hazards, ld, t, e, fake, n, bins, alpha, eps, which,
                     risk, (double*)ws);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(surv_merge_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, blocks, 1.0, out16);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_ple_loss(const float* theta, const float* T, const float* E, int64_t n, double* out2, void* ws, size_t ws_bytes,
                               advmil_stream_t stream_) {
  if (!theta || !T || !E || !out2 || !ws || n <= 0 || n > 0x7fffffff) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_ple_loss_workspace_bytes(n)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(ple_terms_kernel, dim3((unsigned)n), dim3(256), 0, stream, theta, T, E, n, (double*)ws);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(ple_merge_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, n, out2);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_rank_loss_fwd(const float* pred, const float* t, const float* e, int64_t n, float gamma, int l2, int add_weight,
                                    double* state4, float* loss, void* ws, size_t ws_bytes, advmil_stream_t stream_) {
  if (!pred || !t || !e || !state4 || !loss || !ws || n <= 0 || n > 0x7fffffff) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_rank_loss_workspace_bytes(n)) return ADVMIL_EWORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(rank_fwd_anchor_kernel, dim3((unsigned)n), dim3(256), 0, stream, pred, t, e, n, gamma, l2 != 0, add_weight != 0,
                     (double*)ws);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_fwd_merge_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, n, add_weight != 0, state4, loss);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_rank_loss_bwd(const float* pred, const float* t, const float* e, int64_t n, float gamma, int l2, int add_weight,
                                    const double* state4, const float* gout, float* dpred, advmil_stream_t stream_) {
  if (!pred || !t || !e || !state4 || !gout || !dpred || n <= 0 || n > 0x7fffffff) return ADVMIL_EINVAL;
  hipLaunchKernelGGL(rank_bwd_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream_, pred, t, e, n, gamma, l2 != 0,
                     add_weight != 0, state4, gout, dpred);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
