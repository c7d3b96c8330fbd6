// Batched k-means (Lloyd) over the rows of a slab, the cluster ids of `bcb_mode: cluster`: the reference gets
// them offline from tools/deepattnmisl_cluster.py (sklearn KMeans on the CPU); here one iteration is two passes over X. Conventions of
// knn.hip: rows are partitioned into bags by seg_ptr (ops.Segments.ptr), every bag has its own K centres cent[nseg, K, C] (fp32), a
// row meets its own bag's centres only. No atomics anywhere; every sum has a fixed order that depends on the bag alone (never on where
// the bag lies in the slab), so a bag gives the same bits alone and inside a batch, and nothing depends on what outputs or workspace
// held. `active[nseg]` (int32, may be NULL = all): the rows, labels, distances and centres of a bag with active[b] == 0 are not touched.
//
// assign: S^T[centre, row] = cent . X^T with the three-MFMA bf16x3 product over the operand planes of X; the centres are split to
//   hi / lo while they are staged into LDS, where they stay for the whole launch. With the centres as the A operand the accumulator of
//   v_mfma_f32_32x32x16_bf16 has the ROW on the lane and 16 of the 32 centre slots in its registers, in ascending centre order: a lane
//   takes a strict-< running minimum of c_j - 2 s_ij, the two lane halves are merged by (rank, j) -> ties go to the lowest j.
// update: per (bag, chunk of KM_UR rows counted from the bag's first row) the per-cluster column sums in row order, then a fold over
//   the chunks in ascending order, mean = (float)((double)sum / count); an empty cluster keeps its centre.
// seeding (sklearn's greedy k-means++, one pick = two launches over the whole slab): the candidate pass forms, with the MFMA product
//   of assign, the distance of every row to its bag's L trial rows (read from the planes themselves), m_il = min(closest_i, d_il), and
//   the float64 sum of m_il over every chunk of KM_UR rows of the bag; the pick pass folds the chunks (ascending), keeps the trial with
//   the lowest potential, makes its m the new closest, scans it in float64 (chunk carry = the fold of the chunks before, so the last
//   prefix IS the potential) and places the next pick's L draws u * potential in the scan (np.searchsorted side="left", clipped).
#include <float.h>
#include "bf16split.h"
#include "advmil_hip.h"

#define KM_THREADS 256
#define KM_TR 32              // assign: rows per workgroup (the 32 columns of the MFMA tile)
#define KM_CH 64              // assign: feature columns per chunk: lane (r, h) reads the 32 consecutive columns 64 ch + 32 h of row r
#define KM_PAD 8              // halfwords of padding per staged centre row (16 B: the rows of a ds_read_b128 group fall on distinct slots)
#define KM_MAXK 32
#define KM_LDS_MAX 163840     // the 160 KB of a gfx950 CU
#define KM_UT 64              // update: threads per workgroup, a float4 each -> KM_UC columns
#define KM_UC 256
#define KM_UR 128             // update: rows per chunk (two per lane in the count ballots)
#define KM_UG 8               // update: rows per load group

// index of the bag of slab row i: the LAST s with ptr[s] <= i (empty bags are skipped)
__device__ __forceinline__ int km_bag_index(const int64_t* __restrict__ seg_ptr, int nseg, int64_t i) {
  if (!seg_ptr) return 0;
  int a = 0, b = nseg;
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (seg_ptr[m] <= i) a = m; else b = m;
  }
  return a;
}
__device__ __forceinline__ void km_bag_bounds(const int64_t* __restrict__ seg_ptr, int64_t N, int b, int64_t& lo, int64_t& hi) {
  lo = seg_ptr ? seg_ptr[b] : 0;
  hi = seg_ptr ? seg_ptr[b + 1] : N;
  lo = lo < 0 ? 0 : lo;                    // clamped to the slab: no offset array can send a row index outside [0, N)
  hi = hi > N ? N : hi;
}

__device__ __forceinline__ float km_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float km_bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// sum of (hi + lo)^2 over the 8 values of one 16-byte piece of each plane, continuing `acc` (the chain of knn_norms_kernel)
__device__ __forceinline__ float km_norm8(const uint4& h, const uint4& l, float acc) {
  const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float v0 = km_bf16_lo(hw[e]) + km_bf16_lo(lw[e]), v1 = km_bf16_hi(hw[e]) + km_bf16_hi(lw[e]);
    acc = fmaf(v0, v0, acc);
    acc = fmaf(v1, v1, acc);
  }
  return acc;
}

// n_i = fp32 squared norm of row i from its planes: one wave per row, as knn_norms_kernel (same order, same bits)
__global__ __launch_bounds__(KM_THREADS) void kmeans_norms_kernel(const bf16raw* __restrict__ xh, const bf16raw* __restrict__ xl, int64_t ldx,
                                                                   int64_t N, int64_t C, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= N) return;                    // (wave-uniform; no barrier in this kernel)
  float acc = 0.f;
  for (int64_t c = 8 * lane; c < C; c += 8 * 64)
    acc = km_norm8(*(const uint4*)(xh + row * ldx + c), *(const uint4*)(xl + row * ldx + c), acc);
  acc = wave_sum(acc);
  if (lane == 0) norms[row] = acc;
}

// A workgroup (4 waves) owns KM_TR = 32 consecutive slab rows. Wave w forms the partial products of the chunks ch = w, w + 4, ... (the
// next chunk's global loads in flight under the MFMAs); the four partial accumulators are summed in wave order through LDS and wave 0
// selects. k order inside a chunk: k-step s, lane half h, element e <-> column 64 ch + 32 h + 8 s + e, for both operands, so that a
// lane's global read of a chunk is 64 consecutive bytes of each plane. A tile that holds rows of several bags walks them one after the
// other (the centres are re-staged per bag); rows of the other bags are computed and dropped.
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const bf16raw* __restrict__ xh, const bf16raw* __restrict__ xl, int64_t ldx,
                                                                    int64_t N, int64_t C, int K, int nseg, const int64_t* __restrict__ seg_ptr,
                                                                    const int32_t* __restrict__ active, const float* __restrict__ cent,
                                                                    const float* __restrict__ norms, int32_t* __restrict__ labels,
                                                                    float* __restrict__ dist2, int32_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) bf16raw km_lds[];         // c_hi [K][C + KM_PAD] | c_lo [K][C + KM_PAD]
  __shared__ float part[3 * 16 * 64];                                      // partial accumulators of waves 1..3: [wave - 1][register][lane]
  __shared__ float sc[KM_MAXK];                                            // c_j
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int P = (int)C + KM_PAD;
  bf16raw* ch_ = km_lds;
  bf16raw* cl_ = km_lds + (size_t)K * P;
  const int64_t q0 = (int64_t)blockIdx.x * KM_TR;
  const int64_t qlast = (q0 + KM_TR < N ? q0 + KM_TR : N) - 1;
  const int b0 = km_bag_index(seg_ptr, nseg, q0), b1 = km_bag_index(seg_ptr, nseg, qlast);
  const int64_t qi = q0 + r;
  const int64_t qr = qi < N ? qi : N - 1;                 // rows past the slab: a clamped copy, never written
  const int nch = (int)((C + KM_CH - 1) / KM_CH);
  const bool half_last = (C % KM_CH) != 0;                // C % 64 == 32: the last chunk holds 32 columns, 16 per lane half
  const int jr = r < K ? r : K - 1;                       // centre slots >= K: a clamped copy, masked in the selection

  for (int b = b0; b <= b1; ++b) {
    int64_t lo, hi;
    km_bag_bounds(seg_ptr, N, b, lo, hi);
    if (lo >= hi || hi <= q0 || lo > qlast) continue;     // (workgroup-uniform)
    if (active && active[b] == 0) continue;
    __syncthreads();                                      // the previous bag's reads of the centres, of part and of sc are done
    const float* cb = cent + (size_t)b * K * C;
    for (int64_t i4 = tid; i4 < (int64_t)K * (C / 4); i4 += KM_THREADS) {
      const int j = (int)(i4 / (C / 4)), c = 4 * (int)(i4 % (C / 4));
      uint2 vh, vl;
      split4(*(const float4*)(cb + (size_t)j * C + c), vh, vl);
      *(uint2*)(ch_ + j * P + c) = vh;
      *(uint2*)(cl_ + j * P + c) = vl;
    }
    __syncthreads();
    for (int j = w; j < K; j += KM_THREADS / 64) {        // c_j: one wave per centre, the chain of the row norms
      float a = 0.f;
      for (int c = 8 * lane; c < (int)C; c += 8 * 64) a = km_norm8(*(const uint4*)(ch_ + j * P + c), *(const uint4*)(cl_ + j * P + c), a);
      a = wave_sum(a);
      if (lane == 0) sc[j] = a;
    }

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    uint4 gh0, gh1, gh2, gh3, gl0, gl1, gl2, gl3;          // (named, not an array: see knn.hip)
    gh0 = gh1 = gh2 = gh3 = gl0 = gl1 = gl2 = gl3 = make_uint4(0, 0, 0, 0);
#define KM_GLOAD(CHK)                                                                                         \
  do {                                                                                                        \
    const bool hf = half_last && (CHK) == nch - 1;                                                            \
    const int64_t co = (int64_t)(CHK) * KM_CH + (hf ? 16 : 32) * h;                                           \
    const bf16raw* ph = xh + qr * ldx + co;                                                                   \
    const bf16raw* pl = xl + qr * ldx + co;                                                                   \
    gh0 = *(const uint4*)(ph);                                                                                \
    gh1 = *(const uint4*)(ph + 8);                                                                            \
    gl0 = *(const uint4*)(pl);                                                                                \
    gl1 = *(const uint4*)(pl + 8);                                                                            \
    if (!hf) {                                                                                                \
      gh2 = *(const uint4*)(ph + 16);                                                                         \
      gh3 = *(const uint4*)(ph + 24);                                                                         \
      gl2 = *(const uint4*)(pl + 16);                                                                         \
      gl3 = *(const uint4*)(pl + 24);                                                                         \
    }                                                                                                         \
  } while (0)
#define KM_STEP(GH, GL, S)                                                                                    \
  do {                                                                                                        \
    Frag8 ah, al, bh, bl;                                                                                     \
    ah.u = *(const uint4*)(ch_ + jr * P + co + 8 * (S));                                                      \
    al.u = *(const uint4*)(cl_ + jr * P + co + 8 * (S));                                                      \
    bh.u = GH;                                                                                                \
    bl.u = GL;                                                                                                \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bh.v, acc, 0, 0, 0);                                  \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bl.v, acc, 0, 0, 0);                                  \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bh.v, acc, 0, 0, 0);                                  \
  } while (0)
    if (w < nch) KM_GLOAD(w);
    for (int c = w; c < nch; c += KM_THREADS / 64) {
      const bool hf = half_last && c == nch - 1;
      const int co = c * KM_CH + (hf ? 16 : 32) * h;
      const uint4 h0 = gh0, h1 = gh1, h2 = gh2, h3 = gh3, l0 = gl0, l1 = gl1, l2 = gl2, l3 = gl3;
      if (c + KM_THREADS / 64 < nch) KM_GLOAD(c + KM_THREADS / 64);
      KM_STEP(h0, l0, 0);
      KM_STEP(h1, l1, 1);
      if (!hf) {
        KM_STEP(h2, l2, 2);
        KM_STEP(h3, l3, 3);
      }
    }
    if (w > 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) part[((w - 1) * 16 + e) * 64 + lane] = acc[e];
    }
    __syncthreads();                                      // part and sc are complete
    if (w == 0) {
      float best = INFINITY;
      int bj = KM_MAXK;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = (e & 3) + 8 * (e >> 2) + 4 * h;     // ascending in e
        const float s = ((acc[e] + part[(0 * 16 + e) * 64 + lane]) + part[(1 * 16 + e) * 64 + lane]) + part[(2 * 16 + e) * 64 + lane];
        const float rank = fmaf(-2.f, s, sc[j < K ? j : 0]);
        if (j < K && rank < best) { best = rank; bj = j; }
      }
      const float ob = __shfl_xor(best, 32, 64);
      const int oj = __shfl_xor(bj, 32, 64);
      if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      if (h == 0 && qi < N && qi >= lo && qi < hi) {
        if (bj >= K) { bj = 0; best = fmaf(-2.f, 0.f, sc[0]); }          // every rank NaN: slot 0, a defined value
        if (flags) flags[qi] = labels[qi] != bj ? 1 : 0;
        labels[qi] = bj;
        if (dist2) dist2[qi] = fmaxf(0.f, norms[qi] + best);
      }
    }
  }
#undef KM_GLOAD
#undef KM_STEP
}

// changed[b] = the number of rows of bag b whose label moved in the assign launch just before; 0 for an inactive bag. One workgroup
// of KM_CT threads per bag (eight independent loads in flight per thread), integer sums.
#define KM_CT 1024
__global__ __launch_bounds__(KM_CT) void kmeans_changed_kernel(const int32_t* __restrict__ flags, int64_t N, int nseg,
                                                               const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ active,
                                                               int32_t* __restrict__ changed) {
  __shared__ int red[KM_CT / 64];
  const int b = blockIdx.x;
  int64_t lo, hi;
  km_bag_bounds(seg_ptr, N, b, lo, hi);
  int n = 0;
  if (!active || active[b] != 0) {
    for (int64_t i = lo + threadIdx.x; i < hi; i += 8 * KM_CT) {
      int f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = i + e * KM_CT < hi ? flags[i + e * KM_CT] : 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) n += f[e];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < KM_CT / 64; ++w) tot += red[w];
    changed[b] = tot;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// update
// ------------------------------------------------------------------------------------------------------------------------------
// grid (chunk, column tile, bag): the per-cluster sums of KM_UC columns over the rows [lo + KM_UR chunk, + KM_UR) of the bag, in row
// order. Every lane owns four columns of every cluster's LDS accumulator (no two lanes share an address); the label is wave-uniform.
// Rows whose label lies outside [0, K) are skipped. Writes psum[bag][chunk][K][C] (every cluster, zeros too) and, from column tile 0,
// pcnt[bag][chunk][K].
__global__ __launch_bounds__(KM_UT) void kmeans_partial_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int64_t C, int K, int nseg,
                                                               const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ active,
                                                               const int32_t* __restrict__ labels, int mchunk, float* __restrict__ psum,
                                                               int32_t* __restrict__ pcnt) {
  extern __shared__ float4 sacc[];                         // [K][KM_UT]: 1 KB per cluster
  const int b = blockIdx.z, ct = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
  if (active && active[b] == 0) return;
  int64_t lo, hi;
  km_bag_bounds(seg_ptr, N, b, lo, hi);
  const int64_t r0 = lo + (int64_t)chunk * KM_UR;
  if (r0 >= hi) return;
  const int nr = (int)(hi - r0 < KM_UR ? hi - r0 : KM_UR);
  const int64_t col = (int64_t)ct * KM_UC + 4 * t;
  const bool on = col < C;
  for (int j = 0; j < K; ++j) sacc[j * KM_UT + t] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* xp = x + r0 * ldx + (on ? col : 0);
#define KM_ADD(L, V)                                                         \
  if ((unsigned)(L) < (unsigned)K) {                                         \
    float4 a = sacc[(L) * KM_UT + t];                                        \
    a.x += V.x; a.y += V.y; a.z += V.z; a.w += V.w;                          \
    sacc[(L) * KM_UT + t] = a;                                               \
  }
  // groups of KM_UG rows: the next group's loads are in flight under this group's ordered read-modify-writes. A row past the chunk
  // carries label -1 and is skipped.
  float4 v[KM_UG], nx[KM_UG];
  int l[KM_UG], nl[KM_UG];
#pragma unroll
  for (int e = 0; e < KM_UG; ++e) {
    l[e] = e < nr ? labels[r0 + e] : -1;
    v[e] = (on && e < nr) ? *(const float4*)(xp + (int64_t)e * ldx) : make_float4(0.f, 0.f, 0.f, 0.f);
    nl[e] = -1;
    nx[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int i = 0; i < nr; i += KM_UG) {
    if (i + KM_UG < nr) {
#pragma unroll
      for (int e = 0; e < KM_UG; ++e) {
        const int r = i + KM_UG + e;
        nl[e] = r < nr ? labels[r0 + r] : -1;
        nx[e] = (on && r < nr) ? *(const float4*)(xp + (int64_t)r * ldx) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int e = 0; e < KM_UG; ++e) { KM_ADD(l[e], v[e]) }
#pragma unroll
    for (int e = 0; e < KM_UG; ++e) { l[e] = nl[e]; v[e] = nx[e]; }
  }
#undef KM_ADD
  float* out = psum + (((size_t)b * mchunk + chunk) * K) * C;
  if (on)
    for (int j = 0; j < K; ++j) *(float4*)(out + (size_t)j * C + col) = sacc[j * KM_UT + t];
  if (ct == 0) {                                          // counts: a lane holds the labels of rows t and t + 64, one ballot pair per cluster
    const int la = t < nr ? labels[r0 + t] : -1, lb = t + KM_UT < nr ? labels[r0 + t + KM_UT] : -1;
    int mine = 0;
    for (int j = 0; j < K; ++j) {
      const int n = __popcll(__ballot(la == j)) + __popcll(__ballot(lb == j));
      if (t == j) mine = n;
    }
    if (t < K) pcnt[((size_t)b * mchunk + chunk) * K + t] = mine;
  }
}

// grid (column tile, cluster, bag), one wave: folds the chunk partials in ascending chunk order, forms the mean, writes the new centre
// (cent_new may be cent itself: every element is read and written by the same lane), count and this tile's share of the shift.
__global__ __launch_bounds__(KM_UT) void kmeans_fold_kernel(int64_t N, int64_t C, int K, int nseg, const int64_t* __restrict__ seg_ptr,
                                                            const int32_t* __restrict__ active, const float* cent, int mchunk,
                                                            const float* __restrict__ psum, const int32_t* __restrict__ pcnt, float* cent_new,
                                                            int32_t* __restrict__ count, float* __restrict__ pshift, int nct) {
  const int b = blockIdx.z, j = blockIdx.y, ct = blockIdx.x, t = threadIdx.x;
  const int64_t col = (int64_t)ct * KM_UC + 4 * t;
  const bool on = col < C;
  const size_t ci = ((size_t)b * K + j) * C + col;
  float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) old = *(const float4*)(cent + ci);
  float4 nw = old;
  if (!active || active[b] != 0) {
    int64_t lo, hi;
    km_bag_bounds(seg_ptr, N, b, lo, hi);
    int nchunk = (int)((hi - lo + KM_UR - 1) / KM_UR);
    nchunk = nchunk < mchunk ? nchunk : mchunk;          // (a bag longer than max_len: the caller's error, never a read past the workspace)
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int n = 0;
    for (int c0 = 0; c0 < nchunk; c0 += 8) {               // eight chunks' loads in flight, added in ascending chunk order
      float4 p[8];
      int q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool in = c0 + e < nchunk;
        q[e] = in ? pcnt[((size_t)b * mchunk + c0 + e) * K + j] : 0;
        p[e] = (in && on) ? *(const float4*)(psum + (((size_t)b * mchunk + c0 + e) * K + j) * C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c0 + e < nchunk) {
          n += q[e];
          s.x += p[e].x; s.y += p[e].y; s.z += p[e].z; s.w += p[e].w;
        }
    }
    if (n > 0) {
      const double d = (double)n;
      nw = make_float4((float)((double)s.x / d), (float)((double)s.y / d), (float)((double)s.z / d), (float)((double)s.w / d));
    }
    if (ct == 0 && t == 0) count[(size_t)b * K + j] = n;
  }
  if (on) *(float4*)(cent_new + ci) = nw;
  const float dx = nw.x - old.x, dy = nw.y - old.y, dz = nw.z - old.z, dw = nw.w - old.w;
  float sh = fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
  sh = wave_sum(sh);
  if (t == 0) pshift[((size_t)b * K + j) * nct + ct] = sh;
}

// shift2[b] = the sum of the bag's K * nct shares in ascending (cluster, column tile); 0 for an inactive bag
__global__ void kmeans_shift_kernel(int K, int nseg, int nct, const int32_t* __restrict__ active, const float* __restrict__ pshift,
                                    float* __restrict__ shift2) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nseg) return;
  float s = 0.f;
  if (!active || active[b] != 0)
    for (int i = 0; i < K * nct; ++i) s += pshift[(size_t)b * K * nct + i];
  shift2[b] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// greedy k-means++ seeding
// ------------------------------------------------------------------------------------------------------------------------------
#define KM_MAXL 8             // trials per pick (2 + int(ln K) <= 5 at K <= 32): registers 0..3 of the two lane halves hold slots 0..3 | 4..7

// a bag-local row index from device memory, clamped into the bag: no index array can send a read outside [lo, hi)
__device__ __forceinline__ int64_t km_local_row(int32_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : (int64_t)v); }

// grid (chunk of KM_UR rows counted from the BAG's first row, bag). The bag's L trial rows are copied from the planes into LDS and
// are the A operand; wave w owns the 32 rows [32 w, 32 w + 32) of the chunk and walks every feature chunk itself, with one
// accumulator per residue of the chunk index mod 4, summed ((0 + 1) + 2) + 3 -- the partial sums of assign's four waves in assign's
// order, so d_il has the bits kmeans_assign gives for row i against the centre x[cand_l]. Writes candmin[N, L] and, per (bag, chunk),
// cpot[bag][chunk][L] = the float64 sum of the chunk's m_il in row order.
__global__ __launch_bounds__(KM_THREADS) void kmeans_seed_cand_kernel(const bf16raw* __restrict__ xh, const bf16raw* __restrict__ xl, int64_t ldx,
                                                                       int64_t N, int64_t C, int L, int nseg, const int64_t* __restrict__ seg_ptr,
                                                                       int mchunk, const int32_t* __restrict__ cand,
                                                                       const float* __restrict__ closest, const float* __restrict__ norms,
                                                                       float* __restrict__ candmin, double* __restrict__ cpot) {
  extern __shared__ __attribute__((aligned(16))) bf16raw km_lds[];         // t_hi [L][C + KM_PAD] | t_lo [L][C + KM_PAD]
  __shared__ float mlds[KM_UR * KM_MAXL];                                  // m_il of the chunk: [row][L]
  __shared__ float sc[KM_MAXL];                                            // n of the trial rows
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, chunk = blockIdx.x;
  int64_t lo, hi;
  km_bag_bounds(seg_ptr, N, b, lo, hi);
  const int64_t r0 = lo + (int64_t)chunk * KM_UR;
  if (r0 >= hi) return;                                   // (workgroup-uniform)
  const int nr = (int)(hi - r0 < KM_UR ? hi - r0 : KM_UR);
  const int P = (int)C + KM_PAD;
  bf16raw* ch_ = km_lds;
  bf16raw* cl_ = km_lds + (size_t)L * P;
  for (int64_t i8 = tid; i8 < (int64_t)L * (C / 8); i8 += KM_THREADS) {
    const int j = (int)(i8 / (C / 8)), c = 8 * (int)(i8 % (C / 8));
    const int64_t cr = lo + km_local_row(cand[(size_t)b * L + j], hi - lo);
    *(uint4*)(ch_ + j * P + c) = *(const uint4*)(xh + cr * ldx + c);
    *(uint4*)(cl_ + j * P + c) = *(const uint4*)(xl + cr * ldx + c);
  }
  if (tid < L) sc[tid] = norms[lo + km_local_row(cand[(size_t)b * L + tid], hi - lo)];
  __syncthreads();

  const int64_t qi = r0 + 32 * w + r;
  const int64_t qr = qi < hi ? qi : hi - 1;               // rows past the bag: a clamped copy, never written
  const int nch = (int)((C + KM_CH - 1) / KM_CH);
  const bool half_last = (C % KM_CH) != 0;
  const int jr = r < L ? r : L - 1;                       // trial slots >= L: a clamped copy, never written
  if (32 * w < nr) {                                      // (wave-uniform)
    f32x16 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;
    for (int c0 = 0; c0 < nch; c0 += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + k;
        if (c < nch) {
          const bool hf = half_last && c == nch - 1;
          const int co = c * KM_CH + (hf ? 16 : 32) * h;
          const bf16raw* ph = xh + qr * ldx + co;
          const bf16raw* pl = xl + qr * ldx + co;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s < 2 || !hf) {
              Frag8 ah, al, bh, bl;
              ah.u = *(const uint4*)(ch_ + jr * P + co + 8 * s);
              al.u = *(const uint4*)(cl_ + jr * P + co + 8 * s);
              bh.u = *(const uint4*)(ph + 8 * s);
              bl.u = *(const uint4*)(pl + 8 * s);
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bh.v, acc[k], 0, 0, 0);
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bl.v, acc[k], 0, 0, 0);
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bh.v, acc[k], 0, 0, 0);
            }
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = e + 4 * h;
      const float s = ((acc[0][e] + acc[1][e]) + acc[2][e]) + acc[3][e];
      if (j < L && qi < hi) {
        const float d = fmaxf(0.f, norms[qi] + fmaf(-2.f, s, sc[j]));
        const float m = closest ? fminf(closest[qi], d) : d;
        candmin[(size_t)qi * L + j] = m;
        mlds[(32 * w + r) * L + j] = m;
      }
    }
  }
  __syncthreads();
  if (tid < L) {
    double s = 0.0;
    for (int k = 0; k < nr; ++k) s += (double)mlds[k * L + tid];
    cpot[((size_t)b * mchunk + chunk) * L + tid] = s;
  }
}

// grid (chunk, bag), KM_UR threads, one row each. Every workgroup folds the bag's chunk potentials itself (ascending; the value before
// its own chunk is its scan carry), so the launch needs no second pass: pot[b, l], best = the first minimum, row_out[b] = cand[b, best]
// (from chunk 0), closest_i = candmin[i, best], cum_i = carry + the float64 sum of the chunk's closest up to row i in row order. The
// last row's cum is the fold of every chunk: the bag's potential. Draw l of the next pick lands on the first row with
// cum_i >= u_l * potential (the bag's last row when there is none): exactly one row of the bag meets the test, so one thread writes.
__global__ __launch_bounds__(KM_UR) void kmeans_seed_pick_kernel(int64_t N, int L, int nseg, const int64_t* __restrict__ seg_ptr, int mchunk,
                                                                 const int32_t* __restrict__ cand, const float* __restrict__ candmin,
                                                                 const double* __restrict__ cpot, const double* __restrict__ u, int64_t u_stride,
                                                                 int L_next, int64_t* __restrict__ row_out, int64_t row_stride,
                                                                 double* __restrict__ pot, float* __restrict__ closest,
                                                                 int32_t* __restrict__ cand_next) {
  __shared__ double spot[KM_MAXL], spre[KM_MAXL], dcum[KM_UR];
  __shared__ float sv[KM_UR];
  __shared__ int sbest;
  const int b = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
  int64_t lo, hi;
  km_bag_bounds(seg_ptr, N, b, lo, hi);
  const int64_t r0 = lo + (int64_t)chunk * KM_UR;
  if (r0 >= hi) return;                                   // (workgroup-uniform)
  const int nr = (int)(hi - r0 < KM_UR ? hi - r0 : KM_UR);
  int nchunk = (int)((hi - lo + KM_UR - 1) / KM_UR);
  nchunk = nchunk < mchunk ? nchunk : mchunk;
  if (t < L) {
    double s = 0.0, pre = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      if (c == chunk) pre = s;
      s += cpot[((size_t)b * mchunk + c) * L + t];
    }
    spot[t] = s;
    spre[t] = pre;
    if (chunk == 0) pot[(size_t)b * L + t] = s;
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    for (int l = 1; l < L; ++l)
      if (spot[l] < spot[best]) best = l;                 // strict: ties (and NaN) keep the lowest l
    sbest = best;
    if (chunk == 0) row_out[(size_t)b * row_stride] = km_local_row(cand[(size_t)b * L + best], hi - lo);
  }
  __syncthreads();
  const int best = sbest;
  const double total = spot[best], pre = spre[best];
  const int64_t qi = r0 + t;
  if (t < nr) {
    const float v = candmin[(size_t)qi * L + best];
    closest[qi] = v;
    sv[t] = v;
  }
  if (L_next <= 0) return;                                // (uniform) the last pick draws nothing
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < nr; ++k) {
      s += (double)sv[k];
      dcum[k] = pre + s;
    }
  }
  __syncthreads();
  if (t < nr) {
    const double cur = dcum[t], prev = t > 0 ? dcum[t - 1] : pre;
    const bool head = chunk == 0 && t == 0, last = qi == hi - 1;
    for (int l = 0; l < L_next; ++l) {
      const double target = u[(size_t)b * u_stride + l] * total;
      if ((head || !(prev >= target)) && (cur >= target || last)) cand_next[(size_t)b * L_next + l] = (int32_t)(qi - lo);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
static inline bool km_args_bad(int64_t N, int64_t C, int K, int nseg, const int64_t* seg_ptr) {
  return N <= 0 || N >= ((int64_t)1 << 31) || C <= 0 || C % 32 || K < 1 || K > KM_MAXK || nseg < 1 || (nseg > 1 && !seg_ptr);
}
static inline size_t km_up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t km_assign_lds(int64_t C, int K) { return (size_t)2 * K * (C + KM_PAD) * sizeof(bf16raw); }
static const size_t KM_ASSIGN_STATIC = (3 * 16 * 64 + KM_MAXK) * sizeof(float);

extern "C" size_t advmil_kmeans_assign_workspace_bytes(int64_t N, int64_t C, int K) {
  if (N <= 0 || C <= 0 || K < 1 || K > KM_MAXK) return 0;
  return 2 * km_up16((size_t)N * 4);                      // the rows' squared norms | the rows' label-moved flags
}

extern "C" int advmil_kmeans_assign(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int K, int nseg,
                                    const int64_t* seg_ptr, const int32_t* active, const float* cent, int norms_ready, int32_t* labels,
                                    float* dist2, int32_t* changed, void* ws, size_t ws_bytes, advmil_stream_t stream) {
  if (!x_hi || !x_lo || !cent || !labels || km_args_bad(N, C, K, nseg, seg_ptr)) return ADVMIL_EINVAL;
  if (ldx < C || ldx % 8 || (((uintptr_t)x_hi | (uintptr_t)x_lo | (uintptr_t)cent) & 15)) return ADVMIL_EINVAL;
  const size_t lds = km_assign_lds(C, K);
  if (lds + KM_ASSIGN_STATIC > KM_LDS_MAX) return ADVMIL_EINVAL;           // the bag's centres stay in LDS: K (C + 8) <= 37 856
  if (ws_bytes < advmil_kmeans_assign_workspace_bytes(N, C, K)) return ADVMIL_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 3)) return ADVMIL_EINVAL;
  static const int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_assign_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(KM_LDS_MAX - KM_ASSIGN_STATIC));
  if (attr != 0) return attr;
  float* norms = (float*)ws;
  int32_t* flags = (int32_t*)((char*)ws + km_up16((size_t)N * 4));
  if (!norms_ready) {
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)((N + 3) / 4)), dim3(KM_THREADS), 0, (hipStream_t)stream, (const bf16raw*)x_hi,
                       (const bf16raw*)x_lo, ldx, N, C, norms);
    ADVMIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((N + KM_TR - 1) / KM_TR)), dim3(KM_THREADS), lds, (hipStream_t)stream,
                     (const bf16raw*)x_hi, (const bf16raw*)x_lo, ldx, N, C, K, nseg, seg_ptr, active, cent, norms, labels, dist2,
                     changed ? flags : (int32_t*)nullptr);
  ADVMIL_LAUNCH_CHECK();
  if (changed) {
    hipLaunchKernelGGL(kmeans_changed_kernel, dim3((unsigned)nseg), dim3(KM_CT), 0, (hipStream_t)stream, flags, N, nseg, seg_ptr, active,
                       changed);
    ADVMIL_LAUNCH_CHECK();
  }
  return ADVMIL_OK;
}

static inline bool km_len_bad(int64_t N, int64_t max_len) { return max_len <= 0 || max_len > N; }

// the state of a seeding in progress: the rows' squared norms | the chunk potentials [nseg][chunks of KM_UR rows][L] (float64) that the
// candidate pass leaves for the pick pass
static inline bool km_seed_bad(int64_t N, int L, int nseg, const int64_t* seg_ptr, int64_t max_len) {
  return N <= 0 || N >= ((int64_t)1 << 31) || L < 1 || L > KM_MAXL || nseg < 1 || nseg > 65535 || (nseg > 1 && !seg_ptr) || km_len_bad(N, max_len);
}
extern "C" size_t advmil_kmeans_seed_workspace_bytes(int64_t N, int64_t max_len, int L, int nseg) {
  if (N <= 0 || max_len <= 0 || L < 1 || L > KM_MAXL || nseg < 1) return 0;
  return km_up16((size_t)N * 4) + km_up16((size_t)nseg * (size_t)((max_len + KM_UR - 1) / KM_UR) * L * 8);
}

extern "C" int advmil_kmeans_seed_cand(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int L, int nseg,
                                       const int64_t* seg_ptr, int64_t max_len, const int32_t* cand, const float* closest, int norms_ready,
                                       float* candmin, void* ws, size_t ws_bytes, advmil_stream_t stream) {
  if (!x_hi || !x_lo || !cand || !candmin || C <= 0 || C % 32 || km_seed_bad(N, L, nseg, seg_ptr, max_len)) return ADVMIL_EINVAL;
  if (ldx < C || ldx % 8 || (((uintptr_t)x_hi | (uintptr_t)x_lo) & 15) || (((uintptr_t)cand | (uintptr_t)candmin | (uintptr_t)closest) & 3))
    return ADVMIL_EINVAL;
  const size_t lds = (size_t)2 * L * (C + KM_PAD) * sizeof(bf16raw);
  const size_t fixed = (KM_UR * KM_MAXL + KM_MAXL) * sizeof(float);
  if (lds + fixed > KM_LDS_MAX) return ADVMIL_EINVAL;                      // the bag's trial rows stay in LDS
  if (ws_bytes < advmil_kmeans_seed_workspace_bytes(N, max_len, L, nseg)) return ADVMIL_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 15)) return ADVMIL_EINVAL;
  static const int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_seed_cand_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(KM_LDS_MAX - fixed));
  if (attr != 0) return attr;
  float* norms = (float*)ws;
  double* cpot = (double*)((char*)ws + km_up16((size_t)N * 4));
  const int m = (int)((max_len + KM_UR - 1) / KM_UR);
  if (!norms_ready) {
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)((N + 3) / 4)), dim3(KM_THREADS), 0, (hipStream_t)stream, (const bf16raw*)x_hi,
                       (const bf16raw*)x_lo, ldx, N, C, norms);
    ADVMIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kmeans_seed_cand_kernel, dim3((unsigned)m, (unsigned)nseg), dim3(KM_THREADS), lds, (hipStream_t)stream,
                     (const bf16raw*)x_hi, (const bf16raw*)x_lo, ldx, N, C, L, nseg, seg_ptr, m, cand, closest, (const float*)norms, candmin,
                     cpot);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" int advmil_kmeans_seed_pick(int64_t N, int L, int nseg, const int64_t* seg_ptr, int64_t max_len, const int32_t* cand,
                                       const float* candmin, const double* u, int64_t u_stride, int L_next, int64_t* row_out,
                                       int64_t row_stride, double* pot, float* closest, int32_t* cand_next, const void* ws, size_t ws_bytes,
                                       advmil_stream_t stream) {
  if (!cand || !candmin || !row_out || !pot || !closest || km_seed_bad(N, L, nseg, seg_ptr, max_len)) return ADVMIL_EINVAL;
  if (L_next < 0 || L_next > KM_MAXL || row_stride < 1) return ADVMIL_EINVAL;
  if (L_next > 0 && (!u || !cand_next || cand_next == cand || u_stride < L_next)) return ADVMIL_EINVAL;
  if ((((uintptr_t)cand | (uintptr_t)candmin | (uintptr_t)closest | (uintptr_t)cand_next) & 3) ||
      (((uintptr_t)u | (uintptr_t)row_out | (uintptr_t)pot) & 7))
    return ADVMIL_EINVAL;
  if (ws_bytes < advmil_kmeans_seed_workspace_bytes(N, max_len, L, nseg)) return ADVMIL_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 15)) return ADVMIL_EINVAL;
  const double* cpot = (const double*)((const char*)ws + km_up16((size_t)N * 4));
  const int m = (int)((max_len + KM_UR - 1) / KM_UR);
  hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3((unsigned)m, (unsigned)nseg), dim3(KM_UR), 0, (hipStream_t)stream, N, L, nseg, seg_ptr, m,
                     cand, candmin, cpot, u, u_stride, L_next, row_out, row_stride, pot, closest, cand_next);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

extern "C" size_t advmil_kmeans_update_workspace_bytes(int64_t max_len, int64_t C, int K, int nseg) {
  if (max_len <= 0 || C <= 0 || K < 1 || K > KM_MAXK || nseg < 1) return 0;
  const size_t m = (size_t)((max_len + KM_UR - 1) / KM_UR), nct = (size_t)((C + KM_UC - 1) / KM_UC);
  return km_up16((size_t)nseg * m * K * C * 4) + km_up16((size_t)nseg * m * K * 4) + km_up16((size_t)nseg * K * nct * 4);
}

extern "C" int advmil_kmeans_update(const float* x, int64_t ldx, int64_t N, int64_t C, int K, int nseg, const int64_t* seg_ptr,
                                    int64_t max_len, const int32_t* active, const int32_t* labels, const float* cent, float* cent_new,
                                    int32_t* count, float* shift2, void* ws, size_t ws_bytes, advmil_stream_t stream) {
  if (!x || !labels || !cent || !cent_new || !count || !shift2 || km_args_bad(N, C, K, nseg, seg_ptr) || km_len_bad(N, max_len))
    return ADVMIL_EINVAL;
  if (ldx < C || ldx % 4 || (((uintptr_t)x | (uintptr_t)cent | (uintptr_t)cent_new) & 15)) return ADVMIL_EINVAL;
  if (nseg > 65535) return ADVMIL_EINVAL;                                  // bags ride on the grid's z dimension
  if (ws_bytes < advmil_kmeans_update_workspace_bytes(max_len, C, K, nseg)) return ADVMIL_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 15)) return ADVMIL_EINVAL;
  const int m = (int)((max_len + KM_UR - 1) / KM_UR), nct = (int)((C + KM_UC - 1) / KM_UC);
  float* psum = (float*)ws;
  int32_t* pcnt = (int32_t*)((char*)ws + km_up16((size_t)nseg * m * K * C * 4));
  float* pshift = (float*)((char*)pcnt + km_up16((size_t)nseg * m * K * 4));
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)m, (unsigned)nct, (unsigned)nseg), dim3(KM_UT), (size_t)K * KM_UT * sizeof(float4), (hipStream_t)stream, x, ldx, N, C,
                     K, nseg, seg_ptr, active, labels, m, psum, pcnt);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_fold_kernel, dim3((unsigned)nct, (unsigned)K, (unsigned)nseg), dim3(KM_UT), 0, (hipStream_t)stream, N, C, K, nseg,
                     seg_ptr, active, cent, m, (const float*)psum, (const int32_t*)pcnt, cent_new, count, pshift, nct);
  ADVMIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_shift_kernel, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, (hipStream_t)stream, K, nseg, nct, active,
                     (const float*)pshift, shift2);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
