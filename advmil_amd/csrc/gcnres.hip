// Residual block between the GENConv layers of a deep PatchGCN (torch_geometric DeepGCNLayer, block = 'res'; reference
// model/backbone.py:148-168), one row kernel each way:
//   out = keep / (1 - p) * (x + relu(LayerNorm(h)))            h = the layer's GENConv output, x = the previous layer's output
//   bwd: g = dout * keep / (1 - p);  dx (+)= g;  dh = LayerNorm'(g * (LayerNorm(h) > 0));  dgamma / dbeta = column sums
// The keep decision of element (m, n) is drawn at (seed, stream_id, rng_row[m] * d + n) with the hash of advmil_dropout_apply, and the
// backward draws it again: no mask is stored.
//
// A row lives in registers as float4 column groups: d <= 128 gives a row to HALF a wave (lane l of the half holds columns 4 l .. 4 l + 3,
// two rows per wave instruction), wider rows take the whole wave (columns 4 l + 256 c, c < 2: 8 floats per lane at d = 512). Every access
// of h, x, out, dout, dh and dx is 16 bytes per lane. A workgroup of four waves owns 16 consecutive rows, a wave four of them, and all
// loads of the wave's rows go out before the first reduction (the LayerNorm row kernels of pool.hip, from which the statistics --
// centred variance, second centring of rows with a large mean -- are taken).
// x, out, dout and dx carry a row pitch, so they can be column blocks of a wider buffer.
#include "common.h"
#include "sumq.h"
#include "../../include/advmil_hip.h"

#define GCNRES_MAX_D 512
#define GCNRES_BWD_MAXBLK 2048      // the backward's workgroups walk the 16-row regions with this stride: <= 2048 partial rows to merge

template <int LPR>
__device__ __forceinline__ float row_sum(float v) {      // over the LPR lanes that hold one row
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float& at(float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

template <int NV, bool HALF>
__global__ __launch_bounds__(256) void gcn_res_fwd_kernel(const float* __restrict__ h, const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          int64_t N, int64_t d, float p, const uint64_t* __restrict__ seed,
                                                          uint64_t stream_id, const int64_t* __restrict__ rng_row, float* __restrict__ out,
                                                          int64_t ldo, float* __restrict__ mean, float* __restrict__ rstd) {
  constexpr int LPR = HALF ? 32 : 64;      // lanes per row
  constexpr int RPW = 64 / LPR;            // rows per wave instruction
  constexpr int PASS = 4 / RPW;            // a wave owns 4 of the workgroup's 16 rows
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int hf = lane / LPR, l = lane % LPR;
  const bool drop = seed && p > 0.f;
  uint64_t key = 0;
  float ik = 1.f;
  if (drop) { key = rng_key(*seed, stream_id); ik = hw_rcp(1.f - p); }
  const float invd = hw_rcp((float)d);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gm[NV], bt[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int64_t j = 4 * l + 4 * LPR * c;
    gm[c] = j < d ? ld4(gamma + j) : zero4;
    bt[c] = j < d ? ld4(beta + j) : zero4;
  }
  const int64_t n0 = (int64_t)blockIdx.x * 16 + w * 4 + hf;
  float4 hv[PASS][NV], xv[PASS][NV];
#pragma unroll
  for (int t = 0; t < PASS; ++t) {
    const int64_t n = n0 + t * RPW;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int64_t j = 4 * l + 4 * LPR * c;
      const bool ok = n < N && j < d;
      hv[t][c] = ok ? ld4(h + n * d + j) : zero4;
      xv[t][c] = ok ? ld4(x + n * ldx + j) : zero4;
    }
  }
#pragma unroll
  for (int t = 0; t < PASS; ++t) {
    const int64_t n = n0 + t * RPW;
    const bool live = n < N;      // (a dead row computes on zeros and stores nothing: the halves of a wave stay in step)
    float4 (&v)[NV] = hv[t];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    const float mu0 = row_sum<LPR>(s) * invd;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const bool ok = 4 * l + 4 * LPR * c < d;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float& e = at(v[c], i);
        e = ok ? e - mu0 : 0.f;
        s1 += e;
        s2 += e * e;
      }
    }
    const float ve = row_sum<LPR>(s2) * invd + eps;
    const float dm = ln_recentre(row_sum<LPR>(s1) * invd, ve);
    const float rs = hw_rsq(ve - dm * dm);
    if (l == 0 && live) { mean[n] = mu0 + dm; rstd[n] = rs; }
    const int64_t rrow = (drop && rng_row && live) ? rng_row[n] : n;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int64_t j = 4 * l + 4 * LPR * c;
      float f[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop) rng_keep4(key, (uint64_t)(rrow * d + j), p, ik, f);      // (d % 4 == 0 and j % 4 == 0: an aligned group of four)
      float4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float z = (at(v[c], i) - dm) * rs * at(gm[c], i) + at(bt[c], i);
        const float r = at(xv[t][c], i) + (z <= 0.f ? 0.f : z);          // (a NaN stays a NaN, as torch's relu keeps it)
        at(o, i) = drop ? r * f[i] : r;
      }
      if (live && j < d) st4(out + n * ldo + j, o);
    }
  }
}

template <int NV, bool HALF>
__global__ __launch_bounds__(256) void gcn_res_bwd_kernel(const float* __restrict__ dout, int64_t lddo, const float* __restrict__ h,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd, int64_t N,
                                                          int64_t d, float p, const uint64_t* __restrict__ seed, uint64_t stream_id,
                                                          const int64_t* __restrict__ rng_row, float* __restrict__ dh,
                                                          float* __restrict__ dx, int64_t lddx, int dx_accumulate,
                                                          float* __restrict__ partial) {
  constexpr int LPR = HALF ? 32 : 64;
  constexpr int RPW = 64 / LPR;
  constexpr int PASS = 4 / RPW;
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * GCNRES_MAX_D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int hf = lane / LPR, l = lane % LPR;
  const bool drop = seed && p > 0.f;
  uint64_t key = 0;
  float ik = 1.f;
  if (drop) { key = rng_key(*seed, stream_id); ik = hw_rcp(1.f - p); }
  const float invd = hw_rcp((float)d);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gm[NV], bt[NV], ag[NV], ab[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int64_t j = 4 * l + 4 * LPR * c;
    gm[c] = j < d ? ld4(gamma + j) : zero4;
    bt[c] = j < d ? ld4(beta + j) : zero4;
    ag[c] = zero4; ab[c] = zero4;
  }
  const int64_t nreg = (N + 15) / 16;
  for (int64_t g = blockIdx.x; g < nreg; g += gridDim.x) {
    const int64_t n0 = g * 16 + w * 4 + hf;
    float4 hv[PASS][NV], gv[PASS][NV];
    float mua[PASS], rsa[PASS];
#pragma unroll
    for (int t = 0; t < PASS; ++t) {
      const int64_t n = n0 + t * RPW;
      mua[t] = n < N ? mean[n] : 0.f;
      rsa[t] = n < N ? rstd[n] : 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const int64_t j = 4 * l + 4 * LPR * c;
        const bool ok = n < N && j < d;
        hv[t][c] = ok ? ld4(h + n * d + j) : zero4;
        gv[t][c] = ok ? ld4(dout + n * lddo + j) : zero4;
      }
    }
#pragma unroll
    for (int t = 0; t < PASS; ++t) {
      const int64_t n = n0 + t * RPW;
      const bool live = n < N;
      const float mu = mua[t], rs = rsa[t];
      const int64_t rrow = (drop && rng_row && live) ? rng_row[n] : n;
      // the stored mean is rounded to an ulp of ITSELF (3e-5 for rows near 1e3), which would shift x-hat -- and with it the ReLU mask --
      // against the forward's twice-centred row: centre by the mean of h - mean as well
      float s1 = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const bool ok = live && 4 * l + 4 * LPR * c < d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float& e = at(hv[t][c], i);
          e = ok ? e - mu : 0.f;
          s1 += e;
        }
      }
      const float dm = row_sum<LPR>(s1) * invd;
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const int64_t j = 4 * l + 4 * LPR * c;
        const bool ok = live && j < d;
        if (drop) {
          float f[4];
          rng_keep4(key, (uint64_t)(rrow * d + j), p, ik, f);
#pragma unroll
          for (int i = 0; i < 4; ++i) at(gv[t][c], i) *= f[i];
        }
        if (ok) {      // the residual's share: dx (+)= g
          float4 o = gv[t][c];
          if (dx_accumulate) {
            const float4 a = ld4(dx + n * lddx + j);
            o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
          }
          st4(dx + n * lddx + j, o);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xh = ok ? (at(hv[t][c], i) - dm) * rs : 0.f;
          const float z = xh * at(gm[c], i) + at(bt[c], i);
          const float dz = (ok && z > 0.f) ? at(gv[t][c], i) : 0.f;
          const float dxh = dz * at(gm[c], i);
          at(ag[c], i) += dz * xh;
          at(ab[c], i) += dz;
          c1 += dxh;
          c2 += dxh * xh;
          at(hv[t][c], i) = xh;         // (the row's registers now hold xhat and dxhat)
          at(gv[t][c], i) = dxh;
        }
      }
      c1 = row_sum<LPR>(c1) * invd;
      c2 = row_sum<LPR>(c2) * invd;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const int64_t j = 4 * l + 4 * LPR * c;
        float4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) at(o, i) = rs * (at(gv[t][c], i) - c1 - at(hv[t][c], i) * c2);
        if (live && j < d) st4(dh + n * d + j, o);
      }
    }
  }
  // gamma / beta partials of the workgroup: the two halves of a wave (d <= 128) hold the same columns of different rows
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (HALF) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        at(ag[c], i) += __shfl_xor(at(ag[c], i), 32, 64);
        at(ab[c], i) += __shfl_xor(at(ab[c], i), 32, 64);
      }
    }
    const int64_t j = 4 * l + 4 * LPR * c;
    if (hf == 0 && j < d) {
      st4(red + w * 2 * GCNRES_MAX_D + j, ag[c]);
      st4(red + w * 2 * GCNRES_MAX_D + GCNRES_MAX_D + j, ab[c]);
    }
  }
  __syncthreads();
  float* prow = partial + (int64_t)blockIdx.x * 2 * d;
  for (int64_t j = threadIdx.x; j < d; j += 256) {
    constexpr int S = 2 * GCNRES_MAX_D;
    prow[j] = red[j] + red[S + j] + red[2 * S + j] + red[3 * S + j];
    prow[d + j] = red[GCNRES_MAX_D + j] + red[S + GCNRES_MAX_D + j] + red[2 * S + GCNRES_MAX_D + j] + red[3 * S + GCNRES_MAX_D + j];
  }
}

#define GCNRES_DISPATCH(d, kernel, grid, stream, ...)                                                          \
  do {                                                                                                         \
    if ((d) <= 128) hipLaunchKernelGGL((kernel<1, true>), grid, dim3(256), 0, stream, __VA_ARGS__);            \
    else if ((d) <= 256) hipLaunchKernelGGL((kernel<1, false>), grid, dim3(256), 0, stream, __VA_ARGS__);      \
    else hipLaunchKernelGGL((kernel<2, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                      \
  } while (0)

static bool gcnres_shape_ok(int64_t N, int64_t d, float drop_p, const uint64_t* seed) {
  return N > 0 && d >= 4 && d <= GCNRES_MAX_D && (d & 3) == 0 && drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || seed);
}
static bool gcnres_ld_ok(int64_t ld, int64_t d) { return ld >= d && (ld & 3) == 0; }
static inline int gcnres_bwd_blocks(int64_t N) {
  const int64_t nreg = (N + 15) / 16;
  return (int)(nreg < GCNRES_BWD_MAXBLK ? nreg : GCNRES_BWD_MAXBLK);
}

extern "C" int advmil_gcn_res_fwd(const float* h, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int64_t N,
                                  int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* out,
                                  int64_t ldo, float* mean, float* rstd, advmil_stream_t stream) {
  if (!h || !x || !gamma || !beta || !out || !mean || !rstd || !gcnres_shape_ok(N, d, drop_p, seed)) return ADVMIL_EINVAL;
  if (!gcnres_ld_ok(ldx, d) || !gcnres_ld_ok(ldo, d)) return ADVMIL_EINVAL;
  if ((((uintptr_t)h) | ((uintptr_t)x) | ((uintptr_t)gamma) | ((uintptr_t)beta) | ((uintptr_t)out) | ((uintptr_t)mean) | ((uintptr_t)rstd) |
       ((uintptr_t)seed) | ((uintptr_t)rng_row)) & 15)
    return ADVMIL_EINVAL;
  GCNRES_DISPATCH(d, gcn_res_fwd_kernel, dim3((unsigned)((N + 15) / 16)), (hipStream_t)stream, h, x, ldx, gamma, beta, eps, N, d, drop_p,
                  drop_p > 0.f ? seed : nullptr, stream_id, rng_row, out, ldo, mean, rstd);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" size_t advmil_gcn_res_bwd_workspace_bytes(int64_t N, int64_t d) {
  if (N <= 0 || d <= 0) return 0;
  return (size_t)(gcnres_bwd_blocks(N) * 2 * d) * sizeof(float);
}

extern "C" int advmil_gcn_res_bwd(const float* dout, int64_t lddo, const float* h, const float* gamma, const float* beta, const float* mean,
                                  const float* rstd, int64_t N, int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id,
                                  const int64_t* rng_row, float* dh, float* dx, int64_t lddx, int dx_accumulate, float* dgamma, float* dbeta,
                                  int accumulate, void* ws, size_t ws_bytes, advmil_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dout || !h || !gamma || !beta || !mean || !rstd || !dh || !dx || !dgamma || !dbeta || !ws || !gcnres_shape_ok(N, d, drop_p, seed))
    return ADVMIL_EINVAL;
  if (!gcnres_ld_ok(lddo, d) || !gcnres_ld_ok(lddx, d)) return ADVMIL_EINVAL;
  if ((((uintptr_t)dout) | ((uintptr_t)h) | ((uintptr_t)gamma) | ((uintptr_t)beta) | ((uintptr_t)mean) | ((uintptr_t)rstd) | ((uintptr_t)dh) |
       ((uintptr_t)dx) | ((uintptr_t)dgamma) | ((uintptr_t)dbeta) | ((uintptr_t)ws) | ((uintptr_t)seed) | ((uintptr_t)rng_row)) & 15)
    return ADVMIL_EINVAL;
  if (ws_bytes < advmil_gcn_res_bwd_workspace_bytes(N, d)) return ADVMIL_EWORKSPACE;
  const int L = gcnres_bwd_blocks(N);
  float* partial = (float*)ws;
  GCNRES_DISPATCH(d, gcn_res_bwd_kernel, dim3((unsigned)L), stream, dout, lddo, h, gamma, beta, mean, rstd, N, d, drop_p,
                  drop_p > 0.f ? seed : nullptr, stream_id, rng_row, dh, dx, lddx, dx_accumulate, partial);
  ADVMIL_LAUNCH_CHECK();
  return advmil_sumq(stream, partial, L, 2 * d, 2 * d, dgamma, accumulate, dbeta, d);
}
