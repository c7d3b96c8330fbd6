// Exact k-nearest-neighbour edges of WSI patch graphs: the spatial edge set over integer patch coordinates and
// the latent edge set over patch features, the two searches of the reference's tools/patchgcn_graph_s2.py:70-90 (approximate HNSW
// there, exact here). Rows of the slab are partitioned into bags by seg_ptr (ops.Segments.ptr); a node's neighbours come from its own
// bag, ids are bag-local, row i holds its k nearest nodes other than i itself in ascending (squared distance, neighbour id). Self is
// excluded by index, so a duplicate point at distance 0 is a neighbour. Slots a short bag cannot fill hold -1 and the largest finite
// distance of the type. No atomics and no N x N buffer anywhere: every query's running top-k lives in registers, candidates arrive in
// ascending id order, so two runs give identical bits.
//
// Running top-k: KP (8 or 16, the smallest >= k) slots per lane as a fully unrolled compare-and-shift list (static register indices
// only -- a dynamically indexed private array goes to scratch). A candidate enters only if it is STRICTLY smaller than the last slot,
// and is placed behind every slot it ties with: candidates of one list arrive in ascending id, which makes the list (distance, id)
// ordered without ever comparing ids.
#include <float.h>
#include "bf16split.h"
#include "advmil_hip.h"

#define KNN_THREADS 256
#define KNN_SP_CHUNK 1024     // coordinates staged through LDS per pass of the spatial kernel
#define KNN_TQ 128            // latent: query rows per workgroup (32 per wave)
#define KNN_TK 128            // latent: key rows per tile (four 32-row MFMA tiles per wave)
#define KNN_BK 32             // latent: feature columns per staged chunk (two k-steps of v_mfma_f32_32x32x16_bf16)
#define KNN_PITCH 40          // halfwords per staged row: 64 B of data + 16 B pad -> the 16 rows of a ds_read_b128 lane group fall on 16 distinct 16-B slots
#define KNN_ARR (KNN_TK * KNN_PITCH)

// bag of slab row i: the LAST s with ptr[s] <= i (empty bags are skipped); clamped to the slab so that no index array can send a
// key index outside [0, N)
__device__ __forceinline__ void knn_bag_of(const int64_t* __restrict__ seg_ptr, int nseg, int64_t N, int64_t i, int64_t& lo, int64_t& hi) {
  if (!seg_ptr) { lo = 0; hi = N; return; }
  int a = 0, b = nseg;
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (seg_ptr[m] <= i) a = m; else b = m;
  }
  lo = seg_ptr[a];
  hi = seg_ptr[a + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > N ? N : hi;
}

template <int KP, typename T>
__device__ __forceinline__ void knn_insert(T (&D)[KP], int (&I)[KP], T d, int j) {
#pragma unroll
  for (int s = KP - 1; s > 0; --s) {
    if (d < D[s - 1]) { D[s] = D[s - 1]; I[s] = I[s - 1]; }
    else if (d < D[s]) { D[s] = d; I[s] = j; }
  }
  if (d < D[0]) { D[0] = d; I[0] = j; }
}

// ------------------------------------------------------------------------------------------------------------------------------
// spatial: one thread per query row, squared distances exact in int64 (|dx| < 2^31 -> dx^2 + dy^2 < 2^63). A workgroup owns 256
// consecutive slab rows and streams the keys [first row of its first query's bag, end of its last query's bag) through LDS; a lane
// walks only the part of each chunk that lies in its own bag.
// ------------------------------------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(KNN_THREADS) void knn_spatial_kernel(const int2* __restrict__ xy, int64_t N, int k, int nseg,
                                                                   const int64_t* __restrict__ seg_ptr, int32_t* __restrict__ nbr,
                                                                   long long* __restrict__ dist2) {
  __shared__ int2 sxy[KNN_SP_CHUNK];
  const int64_t q0 = (int64_t)blockIdx.x * KNN_THREADS;
  const int64_t qi = q0 + threadIdx.x;
  int64_t lo = 0, hi = 0, kb, ke, t;
  if (qi < N) knn_bag_of(seg_ptr, nseg, N, qi, lo, hi);
  knn_bag_of(seg_ptr, nseg, N, q0, kb, t);
  knn_bag_of(seg_ptr, nseg, N, (q0 + KNN_THREADS < N ? q0 + KNN_THREADS : N) - 1, t, ke);
  const int2 me = qi < N ? xy[qi] : make_int2(0, 0);
  long long D[KP];
  int I[KP];
#pragma unroll
  for (int s = 0; s < KP; ++s) { D[s] = INT64_MAX; I[s] = -1; }
  for (int64_t c0 = kb; c0 < ke; c0 += KNN_SP_CHUNK) {
    const int n = (int)(ke - c0 < KNN_SP_CHUNK ? ke - c0 : KNN_SP_CHUNK);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += KNN_THREADS) sxy[i] = xy[c0 + i];
    __syncthreads();
    const int a = (int)((lo > c0 ? lo : c0) - c0);
    const int b = (int)((hi < c0 + n ? hi : c0 + n) - c0);
    for (int i = a; i < b; ++i) {
      const int2 p = sxy[i];
      const long long dx = (long long)me.x - p.x, dy = (long long)me.y - p.y;
      const long long d = dx * dx + dy * dy;
      if (c0 + i != qi && d < D[KP - 1]) knn_insert<KP, long long>(D, I, d, (int)(c0 + i));
    }
  }
  if (qi < N) {
#pragma unroll
    for (int s = 0; s < KP; ++s)
      if (s < k) {
        nbr[qi * k + s] = I[s] < 0 ? -1 : (int32_t)(I[s] - lo);
        if (dist2) dist2[qi * k + s] = D[s];
      }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// latent: squared norms n_j of the rows from the planes (one wave per row, fp32), then the fused kernel.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float knn_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float knn_bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

__global__ __launch_bounds__(KNN_THREADS) void knn_norms_kernel(const bf16raw* __restrict__ xh, const bf16raw* __restrict__ xl, int64_t ldx,
                                                                 int64_t N, int64_t C, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= N) return;                    // (wave-uniform; no barrier in this kernel)
  float acc = 0.f;
  for (int64_t c = 8 * lane; c < C; c += 8 * 64) {
    const uint4 h = *(const uint4*)(xh + row * ldx + c), l = *(const uint4*)(xl + row * ldx + c);
    const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v0 = knn_bf16_lo(hw[e]) + knn_bf16_lo(lw[e]), v1 = knn_bf16_hi(hw[e]) + knn_bf16_hi(lw[e]);
      acc = fmaf(v0, v0, acc);
      acc = fmaf(v1, v1, acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) norms[row] = acc;
}

// A workgroup (4 waves) owns KNN_TQ consecutive slab rows as queries, wave w rows 32w .. 32w+31, and walks the key tiles (KNN_TK rows,
// aligned to the slab) that cover [start of its first query's bag, end of its last query's bag). Per tile it forms
// S^T[key, query] = Xk . Xq^T with the three-MFMA bf16x3 product (lo.hi + hi.lo + hi.hi, fp32 accumulation) over chunks of KNN_BK
// feature columns staged through LDS (next chunk's global loads in flight under the MFMAs). With the keys as the A operand the
// accumulator of v_mfma_f32_32x32x16_bf16 has the QUERY on the lane (column lane & 31) and 16 keys in its registers (row
// (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): lane (r, h) keeps the running top-k of query r over the keys of its half h, ranked by
// n_j - 2 s_ij, with no cross-lane traffic and in ascending key order. After the last tile the two halves' lists are merged through
// LDS by (rank, id) and written with dist2 = max(0, n_i + n_j - 2 s_ij).
template <int KP>
__global__ __launch_bounds__(KNN_THREADS) void knn_latent_kernel(const bf16raw* __restrict__ xh, const bf16raw* __restrict__ xl, int64_t ldx,
                                                                  int64_t N, int64_t C, int k, int nseg, const int64_t* __restrict__ seg_ptr,
                                                                  const float* __restrict__ norms, int32_t* __restrict__ nbr,
                                                                  float* __restrict__ dist2) {
  __shared__ __attribute__((aligned(16))) bf16raw lds[4 * KNN_ARR];      // q_hi | q_lo | k_hi | k_lo, KNN_TK rows of KNN_PITCH each
  __shared__ float sn[KNN_TK];
  __shared__ float sel[16 * KNN_THREADS];                                // [accumulator register][thread]: lane-private columns
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.x * KNN_TQ;
  const int64_t qi = q0 + 32 * w + r;
  int64_t lo = 0, hi = 0, kb, ke, t_;
  if (qi < N) knn_bag_of(seg_ptr, nseg, N, qi, lo, hi);
  knn_bag_of(seg_ptr, nseg, N, q0, kb, t_);
  knn_bag_of(seg_ptr, nseg, N, (q0 + KNN_TQ < N ? q0 + KNN_TQ : N) - 1, t_, ke);
  const int64_t kt0 = kb / KNN_TK * KNN_TK;
  const int nch = (int)(C / KNN_BK);

  // staging map: piece p of thread tid is the 16-byte segment (tid & 3) of staged row (tid >> 2) + 64 p
  const int srow = tid >> 2, sseg = tid & 3;
  uint4 g0, g1, g2, g3, g4, g5, g6, g7;                // (named, not an array: the array form was kept in scratch memory)
#define KNN_GLOAD(KT, CH)                                                                                     \
  do {                                                                                                        \
    int64_t qa = q0 + srow, qb = qa + 64, ka = (KT) + srow, kc = ka + 64;                                     \
    qa = qa < N ? qa : N - 1; /* rows past the slab: a clamped copy, never a candidate and never a query */   \
    qb = qb < N ? qb : N - 1;                                                                                 \
    ka = ka < N ? ka : N - 1;                                                                                 \
    kc = kc < N ? kc : N - 1;                                                                                 \
    const int64_t co = (int64_t)(CH) * KNN_BK + 8 * sseg;                                                     \
    g0 = *(const uint4*)(xh + qa * ldx + co);                                                                 \
    g1 = *(const uint4*)(xh + qb * ldx + co);                                                                 \
    g2 = *(const uint4*)(xl + qa * ldx + co);                                                                 \
    g3 = *(const uint4*)(xl + qb * ldx + co);                                                                 \
    g4 = *(const uint4*)(xh + ka * ldx + co);                                                                 \
    g5 = *(const uint4*)(xh + kc * ldx + co);                                                                 \
    g6 = *(const uint4*)(xl + ka * ldx + co);                                                                 \
    g7 = *(const uint4*)(xl + kc * ldx + co);                                                                 \
  } while (0)

  float D[KP];
  int I[KP];
#pragma unroll
  for (int s = 0; s < KP; ++s) { D[s] = FLT_MAX; I[s] = -1; }
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  g0 = g1 = g2 = g3 = g4 = g5 = g6 = g7 = make_uint4(0, 0, 0, 0);
  if (kt0 < ke) KNN_GLOAD(kt0, 0);
  for (int64_t kt = kt0; kt < ke; kt += KNN_TK) {
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();                                  // the previous chunk's fragment reads (and the previous tile's sn reads) are done
      {
        const int oa = srow * KNN_PITCH + 8 * sseg, ob = oa + 64 * KNN_PITCH;
        *(uint4*)(lds + 0 * KNN_ARR + oa) = g0;
        *(uint4*)(lds + 0 * KNN_ARR + ob) = g1;
        *(uint4*)(lds + 1 * KNN_ARR + oa) = g2;
        *(uint4*)(lds + 1 * KNN_ARR + ob) = g3;
        *(uint4*)(lds + 2 * KNN_ARR + oa) = g4;
        *(uint4*)(lds + 2 * KNN_ARR + ob) = g5;
        *(uint4*)(lds + 3 * KNN_ARR + oa) = g6;
        *(uint4*)(lds + 3 * KNN_ARR + ob) = g7;
      }
      if (ch == 0 && tid < KNN_TK) sn[tid] = norms[kt + tid < N ? kt + tid : N - 1];
      __syncthreads();
      if (ch + 1 < nch) KNN_GLOAD(kt, ch + 1);
      else if (kt + KNN_TK < ke) KNN_GLOAD(kt + KNN_TK, 0);
#pragma unroll
      for (int ks = 0; ks < KNN_BK / 16; ++ks) {
        const int ko = 16 * ks + 8 * h;
        Frag8 bh, bl;
        bh.u = *(const uint4*)(lds + 0 * KNN_ARR + (32 * w + r) * KNN_PITCH + ko);
        bl.u = *(const uint4*)(lds + 1 * KNN_ARR + (32 * w + r) * KNN_PITCH + ko);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          Frag8 ah, al;
          ah.u = *(const uint4*)(lds + 2 * KNN_ARR + (32 * t + r) * KNN_PITCH + ko);
          al.u = *(const uint4*)(lds + 3 * KNN_ARR + (32 * t + r) * KNN_PITCH + ko);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bh.v, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bl.v, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bh.v, acc[t], 0, 0, 0);
        }
      }
    }
    // selection epilogue of this key tile: 64 candidates per lane, ascending key id. The accumulators pass through a lane-private
    // LDS column so that a rolled loop (one copy of the insertion code per MFMA tile) can walk them: registers cannot be indexed at
    // run time, and 64 unrolled copies of the insertion are 10 minutes of compile time.
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sel[e * KNN_THREADS + tid] = acc[t][e];
#pragma unroll 1
      for (int e = 0; e < 16; ++e) {
        const int row = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int64_t j = kt + row;
        const float rank = fmaf(-2.f, sel[e * KNN_THREADS + tid], sn[row]);
        if (j >= lo && j < hi && j != qi && rank < D[KP - 1]) knn_insert<KP, float>(D, I, rank, (int)j);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  }

  // merge the two halves' lists of every query: lists in LDS, one thread per query
  __syncthreads();
  float* mr = (float*)lds;                               // [256][KP]
  int* mi = (int*)(mr + KNN_THREADS * KP);               // [256][KP]   (2 * 256 * 16 * 4 B = 32 KB <= the 40 KB of staging)
#pragma unroll
  for (int s = 0; s < KP; ++s) { mr[tid * KP + s] = D[s]; mi[tid * KP + s] = I[s]; }
  __syncthreads();
  if (tid < KNN_TQ && q0 + tid < N) {
    const int64_t q = q0 + tid;
    int64_t qlo, qhi;
    knn_bag_of(seg_ptr, nseg, N, q, qlo, qhi);
    const float nq = norms[q];
    const int l0 = ((tid >> 5) * 64 + (tid & 31)) * KP, l1 = l0 + 32 * KP;
    int pa = 0, pb = 0;
    for (int s = 0; s < k; ++s) {                        // pa + pb == s <= k - 1 <= KP - 1: both reads stay inside their lists
      const float ra = mr[l0 + pa], rb = mr[l1 + pb];
      const int ia = mi[l0 + pa], ib = mi[l1 + pb];
      const bool ta = ra < rb || (ra == rb && (unsigned)ia < (unsigned)ib);      // (-1 as unsigned: an empty slot loses every tie)
      const float rr = ta ? ra : rb;
      const int id = ta ? ia : ib;
      pa += ta ? 1 : 0;
      pb += ta ? 0 : 1;
      nbr[q * k + s] = id < 0 ? -1 : (int32_t)(id - qlo);
      if (dist2) dist2[q * k + s] = id < 0 ? FLT_MAX : fmaxf(0.f, nq + rr);
    }
  }
}

static inline bool knn_seg_args_bad(int64_t N, int k, int nseg, const int64_t* seg_ptr, int64_t max_len) {
  return N <= 0 || N >= ((int64_t)1 << 31) || k < 1 || k > 16 || nseg < 1 || (nseg > 1 && !seg_ptr) || max_len <= 0 || max_len > N;
}

extern "C" int advmil_knn_spatial(const int32_t* xy, int64_t N, int k, int nseg, const int64_t* seg_ptr, int64_t max_len, int32_t* nbr,
                                  int64_t* dist2, advmil_stream_t stream) {
  if (!xy || !nbr || knn_seg_args_bad(N, k, nseg, seg_ptr, max_len)) return ADVMIL_EINVAL;
  if ((uintptr_t)xy & 7) return ADVMIL_EINVAL;         // coordinates are read as pairs
  const dim3 grid((unsigned)((N + KNN_THREADS - 1) / KNN_THREADS));
  if (k <= 8)
    hipLaunchKernelGGL(knn_spatial_kernel<8>, grid, dim3(KNN_THREADS), 0, (hipStream_t)stream, (const int2*)xy, N, k, nseg, seg_ptr, nbr,
                       (long long*)dist2);
  else
    hipLaunchKernelGGL(knn_spatial_kernel<16>, grid, dim3(KNN_THREADS), 0, (hipStream_t)stream, (const int2*)xy, N, k, nseg, seg_ptr, nbr,
                       (long long*)dist2);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" size_t advmil_knn_latent_workspace_bytes(int64_t N, int64_t C, int k) {
  if (N <= 0 || C <= 0 || k < 1 || k > 16) return 0;
  return ((size_t)N * sizeof(float) + 15) & ~(size_t)15;       // the rows' squared norms
}

extern "C" int advmil_knn_latent(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int k, int nseg,
                                 const int64_t* seg_ptr, int64_t max_len, int32_t* nbr, float* dist2, void* ws, size_t ws_bytes,
                                 advmil_stream_t stream) {
  if (!x_hi || !x_lo || !nbr || knn_seg_args_bad(N, k, nseg, seg_ptr, max_len)) return ADVMIL_EINVAL;
  if (C <= 0 || C % KNN_BK || ldx < C || ldx % 8 || (((uintptr_t)x_hi | (uintptr_t)x_lo) & 15)) return ADVMIL_EINVAL;
  if (ws_bytes < advmil_knn_latent_workspace_bytes(N, C, k)) return ADVMIL_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 3)) return ADVMIL_EINVAL;
  float* norms = (float*)ws;
  hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((N + 3) / 4)), dim3(KNN_THREADS), 0, (hipStream_t)stream, (const bf16raw*)x_hi,
                     (const bf16raw*)x_lo, ldx, N, C, norms);
  ADVMIL_LAUNCH_CHECK();
  const dim3 grid((unsigned)((N + KNN_TQ - 1) / KNN_TQ));
  if (k <= 8)
    hipLaunchKernelGGL(knn_latent_kernel<8>, grid, dim3(KNN_THREADS), 0, (hipStream_t)stream, (const bf16raw*)x_hi, (const bf16raw*)x_lo, ldx,
                       N, C, k, nseg, seg_ptr, norms, nbr, dist2);
  else
    hipLaunchKernelGGL(knn_latent_kernel<16>, grid, dim3(KNN_THREADS), 0, (hipStream_t)stream, (const bf16raw*)x_hi, (const bf16raw*)x_lo, ldx,
                       N, C, k, nseg, seg_ptr, norms, nbr, dist2);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
