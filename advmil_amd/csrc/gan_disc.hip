// The discrete-time adversarial task (task: disc_gansurv; reference model/model_handler.py:380-384, 399, 444-445, 460, 472-485):
//   advmil_gan_g_loss_disc  the generator loss over a step batch of hazard rows -- SurvMLE (loss/utils.py:98-134) over the visible bags
//                           plus coef * (-mean f_fake) -- value AND analytic gradient in one launch, the discrete counterpart of
//                           advmil_gan_g_loss (csrc/optim.hip);
//   advmil_mask_rows        out = x * mask, the fake pairs' label rows pred * (z <= t) of both phases; its backward is the same launch on
//                           the incoming gradient.
// <= 32 bags x <= 32 bins: one workgroup of one wave, one lane per bag walking its row, every sum in a fixed order (lane 0 adds the
// per-bag terms in bag order): deterministic, no atomics. The reference composes ~20 elementwise / scan / gather ops and autograd as many.
#include "common.h"
#include "../../include/advmil_hip.h"

#define GDISC_MAXB 32
#define GDISC_MAXK 32

// Per bag b, with h = hz[b, :], t = (int)t[b], c = 1 - e[b] (loss/utils.py:124-133):
//   S = cumprod(1 - h) in bin order (fp32), S_padded = [1 | S];
//   unc = -(1 - c) (log max(S_padded[t], eps) + log max(h[t], eps));  cen = -c log max(S_padded[t + 1], eps);
//   term = (1 - alpha) (cen + unc) + alpha unc;   mle = inv_nv * sum_b vis_b term_b.
// d log S_padded[m] / d h_j = -1 / (1 - h_j) for j < m; a log whose argument lies below eps is the constant log(eps): no gradient
// (torch's clamp passes the gradient where the argument is >= the bound). An unclamped product has no zero factor, so the division is safe;
// it is only evaluated (select, not multiply) where it is used.
__global__ __launch_bounds__(64) void gan_g_loss_disc_kernel(const float* __restrict__ hz, const float* __restrict__ t,
                                                             const float* __restrict__ e, const float* __restrict__ vis,
                                                             const float* __restrict__ fake, int B, int K, float alpha, float eps,
                                                             float coef, float inv_nf, float inv_nv, float* __restrict__ out3,
                                                             float* __restrict__ g_hz, float* __restrict__ g_fake) {
  __shared__ float s_term[GDISC_MAXB], s_fake[GDISC_MAXB];
  const int b = threadIdx.x;
  if (b < B) {
    const float* h = hz + b * K;
    float* g = g_hz + b * K;
    int ti = (int)t[b];
    ti = ti < 0 ? 0 : (ti > K - 1 ? K - 1 : ti);     // (validated on the host when the step plan is built; never an address out of the row)
    const float ei = e[b], c = 1.0f - ei, w = 1.0f - c, v = vis ? vis[b] : 1.0f;
    float S = 1.0f, s_t = 1.0f, s_t1 = 1.0f;         // S_padded[t], S_padded[t + 1]
    for (int k = 0; k <= ti; ++k) {
      if (k == ti) s_t = S;
      S *= 1.0f - h[k];
    }
    s_t1 = S;
    const float ht = h[ti];
    const bool on_t = s_t >= eps, on_t1 = s_t1 >= eps, on_h = ht >= eps;
    const float unc = -w * (logf(fmaxf(s_t, eps)) + logf(fmaxf(ht, eps)));
    const float cen = -c * logf(fmaxf(s_t1, eps));
    s_term[b] = v * ((1.0f - alpha) * (cen + unc) + alpha * unc);
    s_fake[b] = fake[b];
    g_fake[b] = -coef * inv_nf;
    const float sc = v * inv_nv;
    const bool live = inv_nv > 0.0f && v != 0.0f;
    for (int k = 0; k < K; ++k) {
      float d_unc = 0.0f, d_cen = 0.0f;
      if (live && k <= ti) {
        const float r = 1.0f / (1.0f - h[k]);
        if (k < ti && on_t) d_unc = w * r;
        if (k == ti && on_h) d_unc = -w / ht;
        if (on_t1) d_cen = c * r;
      }
      g[k] = live ? sc * ((1.0f - alpha) * (d_cen + d_unc) + alpha * d_unc) : 0.0f;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sm = 0.0f, sf = 0.0f;
    for (int i = 0; i < B; ++i) { sm += s_term[i]; sf += s_fake[i]; }
    const float mle = inv_nv > 0.0f ? sm * inv_nv : 0.0f, gen = -sf * inv_nf;
    out3[0] = mle + coef * gen; out3[1] = mle; out3[2] = gen;
  }
}

extern "C" int advmil_gan_g_loss_disc(const float* hz, const float* t, const float* e, const float* vis_mask, const float* fake, int B,
                                      int K, float alpha, float eps, float coef, float inv_nf, float inv_nv, float* out3, float* g_hz,
                                      float* g_fake, advmil_stream_t stream_) {
  if (!hz || !t || !e || !fake || !out3 || !g_hz || !g_fake || B < 1 || B > GDISC_MAXB || K < 1 || K > GDISC_MAXK) return ADVMIL_EINVAL;
  hipLaunchKernelGGL(gan_g_loss_disc_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, hz, t, e, vis_mask, fake, B, K, alpha, eps, coef,
                     inv_nf, inv_nv, out3, g_hz, g_fake);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}

__global__ __launch_bounds__(256) void mask_rows_kernel(const float* __restrict__ x, const float* __restrict__ mask, int64_t n,
                                                        float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = x[i] * mask[i];
}

// out[B, K] = x[B, K] * mask[B, K] (dense rows, out distinct from x). 1 <= B, K and B * K < 2^31.
extern "C" int advmil_mask_rows(const float* x, const float* mask, int64_t B, int64_t K, float* out, advmil_stream_t stream_) {
  if (!x || !mask || !out || B < 1 || K < 1 || B > (int64_t)0x7fffffff / K) return ADVMIL_EINVAL;
  const int64_t n = B * K;
  const int blocks = (int)(n + 255 < 1024 * 256 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(mask_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, x, mask, n, out);
  ADVMIL_LAUNCH_CHECK();
  return ADVMIL_OK;
}
