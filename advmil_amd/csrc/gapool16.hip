// Gated-attention pooling of each consecutive 16 rows (reference model/backbone_utils.py:171-202 GAPoolPatchEmbedding: GAPool over the
// 4x4 patches of a region). A region is rows [16 r, 16 r + 16) of the slab, so the segment of a row is row >> 4: no offsets, no row ids,
// no workspace, no atomics -- one launch each way, capturable.
//     A[16 r + i]  = softmax_i s[16 r + i]                       (max-subtracted; the maximal row's exponential is exactly 1)
//     emb[r, :]    = sum_{i < 16} A[16 r + i] z[16 r + i, :]     (i ascending in one accumulator per column: the bits do not depend on the grid)
// backward, g = demb[r] (+ demb[R + r], dup = 2):
//     t_i = z_i . g,  c = sum_i A_i t_i (i ascending),  ds_i = A_i (t_i - c),  dz_i = A_i g  (added onto dz when dz_accumulate)
// Forward: a wave owns 4 regions per trip. Lane l holds the score of row l & 15 of region l >> 4; max and sum are xor-butterflies over
// the 16 lanes of a region. The 4 d/4 float4 columns of the wave's regions are then dealt over the lanes (item = lane + 64 k -> region
// item / (d/4), column item % (d/4): at d = 128 lanes 0-31 read a 512-byte row of one region, lanes 32-63 of the next), each lane
// walks its column down the 16 rows with the row's weight taken from the lane that holds it.
// Backward: a wave owns one region. LPR = 16 / 32 / 64 lanes cover a row (d <= 64 / 128 / 512), 64 / LPR rows per pass; the row dots
// are xor-butterflies over the LPR lanes.
#include "common.h"
#include "../../include/advmil_hip.h"

#define GAP_MAX_D 512
#define GAP_FWD_BLOCKS_PER_CU 1      // 16 regions per workgroup trip
#define GAP_BWD_BLOCKS_PER_CU 4      //  4 regions per workgroup trip

__device__ __forceinline__ float4 gap_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__global__ __launch_bounds__(256) void gapool16_fwd_kernel(const float* __restrict__ s, const float* __restrict__ z, int64_t ldz, int64_t R,
                                                           int64_t d, float* __restrict__ A, float* __restrict__ emb, int dup) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int C4 = (int)(d >> 2), items = 4 * C4;
  const int64_t stride = (int64_t)gridDim.x * 16;
  int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 4;            // wave-uniform: every lane of a wave makes the same trips
  float sv = (base + g < R) ? s[(base + g) * 16 + li] : 0.f;
  for (; base < R; base += stride) {
    const int64_t r = base + g;
    float m = sv;
    m = fmaxf(m, __shfl_xor(m, 8, 64)); m = fmaxf(m, __shfl_xor(m, 4, 64));
    m = fmaxf(m, __shfl_xor(m, 2, 64)); m = fmaxf(m, __shfl_xor(m, 1, 64));
    // (a NaN score: fmaxf drops it from m, sv == m is false, exp(NaN) = NaN -> the sum, every weight and emb[r] are NaN)
    const float e = (sv == m) ? 1.f : hw_exp(sv - m);
    float sum = e;
    sum += __shfl_xor(sum, 8, 64); sum += __shfl_xor(sum, 4, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 1, 64);
    const float a = e / sum;
    if (r < R) A[r * 16 + li] = a;
    // the next trip's scores travel under this trip's walk over z
    const int64_t nb = base + stride;
    const float sn = (nb + g < R) ? s[(nb + g) * 16 + li] : 0.f;
    for (int k0 = 0; k0 < items; k0 += 64) {
      const int it = k0 + lane;
      const int rg = it < items ? it / C4 : 0;
      const int c = it - rg * C4;
      const int64_t rr = base + rg;
      const bool ok = it < items && rr < R;
      const float* zp = z + (rr * 16) * ldz + c * 4;
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = ok ? gap_ld4(zp + i * ldz) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float ai = __shfl(a, rg * 16 + i, 64);
        acc.x += ai * v[i].x; acc.y += ai * v[i].y; acc.z += ai * v[i].z; acc.w += ai * v[i].w;
      }
      if (ok) {
        *reinterpret_cast<float4*>(emb + rr * d + c * 4) = acc;
        if (dup == 2) *reinterpret_cast<float4*>(emb + (R + rr) * d + c * 4) = acc;
      }
    }
    sv = sn;
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void gapool16_bwd_kernel(const float* __restrict__ demb, const float* __restrict__ A, const float* __restrict__ z,
                                                           int64_t ldz, int64_t R, int64_t d, int dup, float* __restrict__ ds,
                                                           float* __restrict__ dz, int accumulate) {
  constexpr int RPP = 64 / LPR;                 // rows per pass
  constexpr int NP = 16 / RPP;                  // passes per region
  constexpr int KMAX = LPR == 64 ? GAP_MAX_D / 256 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, cl = lane % LPR, li = lane & 15;
  const int C4 = (int)(d >> 2);
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < R; r += (int64_t)gridDim.x * 4) {      // wave-uniform
    float4 g[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = cl + 64 * k;
      g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C4) {
        g[k] = gap_ld4(demb + r * d + c * 4);
        if (dup == 2) {
          const float4 h = gap_ld4(demb + (R + r) * d + c * 4);
          g[k].x += h.x; g[k].y += h.y; g[k].z += h.z; g[k].w += h.w;
        }
      }
    }
    const float a = A[r * 16 + li];             // every 16-lane group holds the region's 16 weights
    float4 v[NP][KMAX];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int c = cl + 64 * k;
        v[p][k] = c < C4 ? gap_ld4(z + (r * 16 + p * RPP + sub) * ldz + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    float t = 0.f;                              // t of row lane & 15
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) part += (v[p][k].x * g[k].x + v[p][k].y * g[k].y) + (v[p][k].z * g[k].z + v[p][k].w * g[k].w);
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      // the lanes of row group `sub` now hold t of row p RPP + sub; row j = lane & 15 is pass j / RPP, group j % RPP
      const float got = __shfl(part, (li % RPP) * LPR, 64);
      if (li / RPP == p) t = got;
    }
    const float at = a * t;
    float cs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) cs += __shfl(at, i, 64);
    if (lane < 16) ds[r * 16 + lane] = a * (t - cs);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int i = p * RPP + sub;
      const float ai = __shfl(a, i, 64);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int c = cl + 64 * k;
        if (c < C4) {
          float* const q = dz + (r * 16 + i) * d + c * 4;
          float4 o = make_float4(ai * g[k].x, ai * g[k].y, ai * g[k].z, ai * g[k].w);
          if (accumulate) {
            const float4 old = gap_ld4(q);
            o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
          }
          *reinterpret_cast<float4*>(q) = o;
        }
      }
    }
  }
}

// compute units of the current device (asked once; nothing here synchronises, so the entry points stay capturable)
static int gap_cu_count() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      n = 256;
    }
    cus = n;
  }
  return cus;
}

static bool gap_shape_ok(int64_t N, int64_t d, int64_t ldz, int dup) {
  return N > 0 && (N & 15) == 0 && d > 0 && d <= GAP_MAX_D && (d & 3) == 0 && ldz >= d && (ldz & 3) == 0 && (dup == 1 || dup == 2);
}

extern "C" int advmil_gapool16_fwd(const float* s, const float* z, int64_t ldz, int64_t N, int64_t d, float* A, float* emb, int dup,
                                   advmil_stream_t stream) {
  if (!s || !z || !A || !emb || !gap_shape_ok(N, d, ldz, dup)) return ADVMIL_EINVAL;
  if ((((uintptr_t)z) | ((uintptr_t)emb)) & 15) return ADVMIL_EINVAL;
  if ((((uintptr_t)s) | ((uintptr_t)A)) & 3) return ADVMIL_EINVAL;
  const int64_t R = N / 16;
  const int64_t want = (R + 15) / 16, cap = (int64_t)gap_cu_count() * GAP_FWD_BLOCKS_PER_CU;
  hipLaunchKernelGGL(gapool16_fwd_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, (hipStream_t)stream, s, z, ldz, R, d, A, emb,
                     dup);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_gapool16_bwd(const float* demb, const float* A, const float* z, int64_t ldz, int64_t N, int64_t d, int dup, float* ds,
                                   float* dz, int dz_accumulate, advmil_stream_t stream) {
  if (!demb || !A || !z || !ds || !dz || !gap_shape_ok(N, d, ldz, dup)) return ADVMIL_EINVAL;
  if ((((uintptr_t)demb) | ((uintptr_t)z) | ((uintptr_t)dz)) & 15) return ADVMIL_EINVAL;
  if ((((uintptr_t)A) | ((uintptr_t)ds)) & 3) return ADVMIL_EINVAL;
  const int64_t R = N / 16;
  const int64_t want = (R + 3) / 4, cap = (int64_t)gap_cu_count() * GAP_BWD_BLOCKS_PER_CU;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  const int acc = dz_accumulate != 0;
  if (d <= 64) hipLaunchKernelGGL((gapool16_bwd_kernel<16>), grid, dim3(256), 0, (hipStream_t)stream, demb, A, z, ldz, R, d, dup, ds, dz, acc);
  else if (d <= 128) hipLaunchKernelGGL((gapool16_bwd_kernel<32>), grid, dim3(256), 0, (hipStream_t)stream, demb, A, z, ldz, R, d, dup, ds, dz, acc);
  else hipLaunchKernelGGL((gapool16_bwd_kernel<64>), grid, dim3(256), 0, (hipStream_t)stream, demb, A, z, ldz, R, d, dup, ds, dz, acc);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
