// cilfw — PODNet's local similarity classifier (multi-proxy cosine head) and
// its NCA loss for gfx950 (definitions: cilfw/ops/lsc.py).
//
// sims (M, C K) bf16 are pure cosines, class c's K proxies at columns
// c K .. c K + K - 1; sigma[0] fp32 on the device; gamma, margin host floats.
//   lsc_reduce_fwd  per (row, class): e_k = exp(gamma s_k - max_k gamma s_k),
//                   Z = sum_k e_k, yhat = (sum_k e_k s_k) / Z;
//                   logits = bf16(sigma yhat), yhat kept in fp32
//   lsc_reduce_bwd  dsims[k] = ((sigma g) / Z) e_k (1 + gamma (s_k - yhat)),
//                   e_k and Z recomputed from sims, yhat read back;
//                   rows[m] = sum_c g_c yhat_c (cos_sum adds the rows: dsigma)
// logits (M, C) bf16, targets (M) int64; row m is skipped iff its target lies
// outside 0..C-1, otherwise y = targets[m], sm = fp32(sigma margin):
//   nca_fwd         mx = max_{i != y} l_i, lse = mx + log sum_{i != y}
//                   exp(l_i - mx), h = lse - (l_y - sm), active = h > 0;
//                   a skipped row gets h = lse = 0, active = 0
//   nca_finalize    A = sum active; fin = {(1/M) sum_active h, 1/M,
//                   (margin A) (1/M)}, nact = A
//   nca_bwd         active row: dlogits[i] = (up/M) exp(l_i - lse) for
//                   i != y, dlogits[y] = -up/M; every other row 0;
//                   dsig[0] = up fin[2]
//
// One wave per row, four rows per 256-thread block, as in cosine.hip and
// mrank.hip. In the reduce each lane owns whole classes (lane, lane + 64,
// ...), so the K-way softmax is lane-local; neither the class stride 2K
// bytes nor the row strides are 16-byte aligned in general, so every access
// is one bf16 (or one fp32) per lane. fp32 arithmetic, no LDS outside the
// finalize tree, no atomics; every sum has an order fixed by the shape alone,
// so two launches are bit-identical. sigma and the upstream are read from
// device memory: a captured step replays with their current values.

#include "common.h"

#define NT 256
#define LSC_ROWS (NT / WAVE)
#define LSC_KMAX 16

// a * b rounded on its own (never contracted into an fma by the caller)
DEV float lsc_mul_rn(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

DEV float lsc_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

DEV float lsc_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// One class: its K cosines into s[], e_k into e[]; -> Z. K is wave-uniform.
DEV float lsc_softmax_terms(const bf16_t* __restrict__ p, int K, float gamma,
                            float* s, float* e) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < LSC_KMAX; ++k) {
    s[k] = 0.f;
    if (k < K) {
      s[k] = bf2f(p[k]);
      mx = fmaxf(mx, lsc_mul_rn(gamma, s[k]));
    }
  }
  float Z = 0.f;
#pragma unroll
  for (int k = 0; k < LSC_KMAX; ++k) {
    e[k] = 0.f;
    if (k < K) {
      e[k] = __expf(lsc_mul_rn(gamma, s[k]) - mx);
      Z += e[k];
    }
  }
  return Z;  // >= 1: the maximum contributes exp(0)
}

// ------------------------------------------------------------- lsc_reduce_fwd

__global__ __launch_bounds__(NT)
void lsc_reduce_fwd_kernel(const bf16_t* __restrict__ sims,
                           const float* __restrict__ sigma,
                           bf16_t* __restrict__ logits,
                           float* __restrict__ yhat, int M, int C, int K,
                           float gamma) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LSC_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;  // whole waves leave; there is no barrier below
  const float sg = sigma[0];
  const bf16_t* sr = sims + (long)row * C * K;
  for (int c = lane; c < C; c += WAVE) {
    float s[LSC_KMAX], e[LSC_KMAX];
    const float Z = lsc_softmax_terms(sr + (long)c * K, K, gamma, s, e);
    float num = 0.f;
#pragma unroll
    for (int k = 0; k < LSC_KMAX; ++k)
      if (k < K) num += e[k] * s[k];
    const float y = num / Z;
    yhat[(long)row * C + c] = y;
    logits[(long)row * C + c] = f2bf(sg * y);
  }
}

// ------------------------------------------------------------- lsc_reduce_bwd

__global__ __launch_bounds__(NT)
void lsc_reduce_bwd_kernel(const bf16_t* __restrict__ sims,
                           const float* __restrict__ yhat,
                           const bf16_t* __restrict__ g,
                           const float* __restrict__ sigma,
                           bf16_t* __restrict__ dsims,
                           float* __restrict__ rows, int M, int C, int K,
                           float gamma) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LSC_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  const float sg = sigma[0];
  const bf16_t* sr = sims + (long)row * C * K;
  bf16_t* dr = dsims + (long)row * C * K;
  float acc = 0.f;
  for (int c = lane; c < C; c += WAVE) {
    const float gc = bf2f(g[(long)row * C + c]);
    const float y = yhat[(long)row * C + c];
    acc += gc * y;
    float s[LSC_KMAX], e[LSC_KMAX];
    const float Z = lsc_softmax_terms(sr + (long)c * K, K, gamma, s, e);
    const float q = (sg * gc) / Z;
    bf16_t* dp = dr + (long)c * K;
#pragma unroll
    for (int k = 0; k < LSC_KMAX; ++k)
      if (k < K) dp[k] = f2bf(q * e[k] * (1.f + gamma * (s[k] - y)));
  }
  acc = lsc_wave_sum(acc);
  if (lane == 0) rows[row] = acc;
}

// -------------------------------------------------------------------- nca_fwd

__global__ __launch_bounds__(NT)
void nca_fwd_kernel(const bf16_t* __restrict__ logits,
                    const long* __restrict__ targets,
                    const float* __restrict__ sigma, float* __restrict__ h,
                    float* __restrict__ lse, int* __restrict__ active, int M,
                    int C, float margin) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LSC_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  const long t = targets[row];
  if (t < 0 || t >= C) {  // wave-uniform: a skipped row, nothing read at t
    if (lane == 0) {
      h[row] = 0.f;
      lse[row] = 0.f;
      active[row] = 0;
    }
    return;
  }
  const bf16_t* lr = logits + (long)row * C;
  const int y = (int)t;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += WAVE)
    if (c != y) mx = fmaxf(mx, bf2f(lr[c]));
  mx = lsc_wave_max(mx);  // C >= 2: at least one negative
  float se = 0.f;
  for (int c = lane; c < C; c += WAVE)
    if (c != y) se += __expf(bf2f(lr[c]) - mx);
  se = lsc_wave_sum(se);
  if (lane == 0) {
    const float l = mx + __logf(se);
    const float sm = lsc_mul_rn(sigma[0], margin);
    const float hv = l - (bf2f(lr[y]) - sm);
    h[row] = hv;
    lse[row] = l;
    active[row] = hv > 0.f ? 1 : 0;  // 0 for a NaN
  }
}

// --------------------------------------------------------------- nca_finalize
// One block: strided chains, then a fixed LDS tree (mrank_finalize's shape).

__global__ __launch_bounds__(NT)
void nca_finalize_kernel(const float* __restrict__ h,
                         const int* __restrict__ active,
                         float* __restrict__ fin, int* __restrict__ nact,
                         int M, float margin) {
  __shared__ float red_h[NT];
  __shared__ int red_n[NT];
  float s = 0.f;
  int n = 0;
  for (int i = threadIdx.x; i < M; i += NT) {
    const int a = active[i] == 1 ? 1 : 0;
    s += a ? h[i] : 0.f;
    n += a;
  }
  red_h[threadIdx.x] = s;
  red_n[threadIdx.x] = n;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red_h[threadIdx.x] += red_h[threadIdx.x + o];
      red_n[threadIdx.x] += red_n[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float inv = 1.f / (float)M;
    const int A = red_n[0];
    nact[0] = A;
    fin[0] = lsc_mul_rn(red_h[0], inv);
    fin[1] = inv;
    fin[2] = lsc_mul_rn(lsc_mul_rn(margin, (float)A), inv);
  }
}

// -------------------------------------------------------------------- nca_bwd
// Writes the whole dlogits row: softmax over the negatives and -up/M at the
// target for an active row, zeros for every other row.

__global__ __launch_bounds__(NT)
void nca_bwd_kernel(const bf16_t* __restrict__ logits,
                    const long* __restrict__ targets,
                    const float* __restrict__ lse,
                    const int* __restrict__ active,
                    const float* __restrict__ fin,
                    const float* __restrict__ up,
                    bf16_t* __restrict__ dlogits, float* __restrict__ dsig,
                    int M, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LSC_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  const float u = up[0];
  if (row == 0 && lane == 0) dsig[0] = lsc_mul_rn(u, fin[2]);
  const float gq = lsc_mul_rn(u, fin[1]);
  const long t = targets[row];
  const bool act = active[row] == 1 && t >= 0 && t < C;  // wave-uniform
  const float l = act ? lse[row] : 0.f;
  const bf16_t neg = f2bf(-gq);
  const bf16_t* lr = logits + (long)row * C;
  bf16_t* dr = dlogits + (long)row * C;
  for (int c = lane; c < C; c += WAVE) {
    bf16_t o = 0;
    if (act)
      o = c == (int)t ? neg : f2bf(lsc_mul_rn(gq, __expf(bf2f(lr[c]) - l)));
    dr[c] = o;
  }
}

static bool lsc_shape_ok(int M, int C, int K) {
  return M >= 1 && C >= 1 && K >= 1 && K <= LSC_KMAX &&
         (long)C * K < (long)INT32_MAX - WAVE;
}

static bool nca_shape_ok(int M, int C) {
  return M >= 1 && C >= 2 && C < INT32_MAX - WAVE;
}

extern "C" {

// 1 when the reduce launchers accept the shape: M >= 1, C >= 1,
// 1 <= K <= 16, C K < 2^31 - 64
int cilfw_lsc_supported(int M, int C, int K) {
  return lsc_shape_ok(M, C, K) ? 1 : 0;
}

// 1 when the NCA launchers accept the shape: M >= 1, C >= 2
int cilfw_nca_supported(int M, int C) { return nca_shape_ok(M, C) ? 1 : 0; }

// sims bf16 (M, C K), sigma fp32 (1) on the device -> logits bf16 (M, C),
// yhat fp32 (M, C). Every element is written. Returns 0, or 1 when the
// arguments are refused (no launch).
int cilfw_lsc_reduce_fwd(const void* sims, const void* sigma, void* logits,
                         void* yhat, int M, int C, int K, float gamma,
                         void* stream) {
  if (!lsc_shape_ok(M, C, K) || !(gamma >= 0.f)) return 1;
  hipLaunchKernelGGL(lsc_reduce_fwd_kernel, dim3(cdiv(M, LSC_ROWS)), dim3(NT),
                     0, (hipStream_t)stream, (const bf16_t*)sims,
                     (const float*)sigma, (bf16_t*)logits, (float*)yhat, M, C,
                     K, gamma);
  return 0;
}

// sims, yhat as above, g bf16 (M, C) -> dsims bf16 (M, C K), rows fp32 (M) =
// sum_c g_c yhat_c. Every element is written.
int cilfw_lsc_reduce_bwd(const void* sims, const void* yhat, const void* g,
                         const void* sigma, void* dsims, void* rows, int M,
                         int C, int K, float gamma, void* stream) {
  if (!lsc_shape_ok(M, C, K) || !(gamma >= 0.f)) return 1;
  hipLaunchKernelGGL(lsc_reduce_bwd_kernel, dim3(cdiv(M, LSC_ROWS)), dim3(NT),
                     0, (hipStream_t)stream, (const bf16_t*)sims,
                     (const float*)yhat, (const bf16_t*)g,
                     (const float*)sigma, (bf16_t*)dsims, (float*)rows, M, C,
                     K, gamma);
  return 0;
}

// logits bf16 (M, C), targets int64 (M), sigma fp32 (1) on the device -> h,
// lse fp32 (M), active int32 (M), fin fp32 (3) = {loss, 1/M, dsigma for
// upstream 1}, nact int32 (1). Every element is written.
int cilfw_nca_fwd(const void* logits, const void* targets, const void* sigma,
                  void* h, void* lse, void* active, void* fin, void* nact,
                  int M, int C, float margin, void* stream) {
  if (!nca_shape_ok(M, C) || !(margin >= 0.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nca_fwd_kernel, dim3(cdiv(M, LSC_ROWS)), dim3(NT), 0, st,
                     (const bf16_t*)logits, (const long*)targets,
                     (const float*)sigma, (float*)h, (float*)lse,
                     (int*)active, M, C, margin);
  hipLaunchKernelGGL(nca_finalize_kernel, dim3(1), dim3(NT), 0, st,
                     (const float*)h, (const int*)active, (float*)fin,
                     (int*)nact, M, margin);
  return 0;
}

// logits, targets and lse, active, fin as written by cilfw_nca_fwd; up: 1
// fp32 on the device -> dlogits bf16 (M, C), dsig fp32 (1). Every element is
// written.
int cilfw_nca_bwd(const void* logits, const void* targets, const void* lse,
                  const void* active, const void* fin, const void* up,
                  void* dlogits, void* dsig, int M, int C, void* stream) {
  if (!nca_shape_ok(M, C)) return 1;
  hipLaunchKernelGGL(nca_bwd_kernel, dim3(cdiv(M, LSC_ROWS)), dim3(NT), 0,
                     (hipStream_t)stream, (const bf16_t*)logits,
                     (const long*)targets, (const float*)lse,
                     (const int*)active, (const float*)fin, (const float*)up,
                     (bf16_t*)dlogits, (float*)dsig, M, C);
  return 0;
}

}  // extern "C"
