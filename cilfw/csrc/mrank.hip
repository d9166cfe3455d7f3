// cilfw — LUCIR's margin-ranking loss over the cosine head's logits for
// gfx950 (definition: cilfw/ops/margin.py).
//
// logits (M, C) bf16 = sigma z, targets (M) int64, sigma[0] fp32 on the
// device. Row m is an old row iff 0 <= targets[m] < known. For an old row
// a = logits[m, targets[m]] and n_1..n_k at classes c_1..c_k are the k
// largest of logits[m, known:C], descending, ties to the lower class index;
// v_j = fp32(sigma margin) - (a - n_j); pair j is active iff v_j > 0.
//   mrank_fwd       per row: rho = sum_j max(v_j, 0), dsum = sum_active
//                   (a - n_j), old = 1/0, sel[j] = c_j if active else -1
//   mrank_finalize  N = sum old, s = 1/sigma (0 for sigma <= 0),
//                   q = s / (k max(N, 1)); fin = {q sum rho, q, s q sum dsum}
//   mrank_bwd       dlogits[m, c_j] = +up q for an active pair,
//                   dlogits[m, targets[m]] = -up q A_m, every other element
//                   0; dsig[0] = up fin[2]
//
// One wave per row, four rows per 256-thread block, as in cosine.hip; the
// row stride C is not 16-byte aligned in general, so logits are read and
// dlogits written one bf16 per lane (coalesced 128-byte wave accesses). Each
// lane keeps the sorted top-8 of the classes it sweeps in registers; k rounds
// of a wave arg-max on (value, lower index) merge the 64 lists. fp32
// arithmetic, no LDS outside the finalize tree, no atomics; every sum has an
// order fixed by the shape alone, so two launches are bit-identical. sigma,
// N, q and the upstream are read from device memory: a captured step replays
// with their current values.

#include "common.h"

#include <limits.h>

#define NT 256
#define MR_ROWS (NT / WAVE)
#define MR_KMAX 8

// a * b rounded on its own (never contracted into an fma by the caller)
DEV float mr_mul_rn(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

// ------------------------------------------------------------------ mrank_fwd

__global__ __launch_bounds__(NT)
void mrank_fwd_kernel(const bf16_t* __restrict__ logits,
                      const long* __restrict__ targets,
                      const float* __restrict__ sigma,
                      float* __restrict__ rho, float* __restrict__ dsum,
                      int* __restrict__ old, int* __restrict__ sel, int M,
                      int C, int known, int k, float margin) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * MR_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;  // whole waves leave; there is no barrier below
  const long t = targets[row];
  int* srow = sel + (long)row * k;
  if (t < 0 || t >= known) {  // wave-uniform: not an old row
    if (lane < k) srow[lane] = -1;
    if (lane == 0) {
      rho[row] = 0.f;
      dsum[row] = 0.f;
      old[row] = 0;
    }
    return;
  }
  const bf16_t* lr = logits + (long)row * C;
  const float a = bf2f(lr[t]);
  const float sm = mr_mul_rn(sigma[0], margin);

  // this lane's classes known + lane, + 64, ... in ascending order: a strict
  // '>' insert keeps equal values in ascending class order
  float tv[MR_KMAX];
  int ti[MR_KMAX];
#pragma unroll
  for (int j = 0; j < MR_KMAX; ++j) {
    tv[j] = -INFINITY;
    ti[j] = INT_MAX;
  }
  for (int c = known + lane; c < C; c += WAVE) {
    const float x = bf2f(lr[c]);
#pragma unroll
    for (int j = MR_KMAX - 1; j >= 1; --j) {
      const bool above = x > tv[j - 1];  // x lands above slot j: shift down
      const bool here = x > tv[j];
      tv[j] = above ? tv[j - 1] : (here ? x : tv[j]);
      ti[j] = above ? ti[j - 1] : (here ? c : ti[j]);
    }
    const bool top = x > tv[0];
    tv[0] = top ? x : tv[0];
    ti[0] = top ? c : ti[0];
  }

  float r = 0.f, d = 0.f;
  for (int j = 0; j < k; ++j) {
    // wave arg-max of the list heads on (value, lower index): a total order,
    // so the butterfly leaves the same pair in every lane
    float bv = tv[0];
    int bi = ti[0];
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (ti[0] == bi) {  // the owner pops its head (class indices are unique)
#pragma unroll
      for (int e = 0; e < MR_KMAX - 1; ++e) {
        tv[e] = tv[e + 1];
        ti[e] = ti[e + 1];
      }
      tv[MR_KMAX - 1] = -INFINITY;
      ti[MR_KMAX - 1] = INT_MAX;
    }
    const float diff = a - bv;
    const float v = sm - diff;
    const bool active = v > 0.f;  // false for a NaN and for an empty slot
    if (active) {
      r += v;
      d += diff;
    }
    if (lane == 0) srow[j] = active ? bi : -1;
  }
  if (lane == 0) {
    rho[row] = r;
    dsum[row] = d;
    old[row] = 1;
  }
}

// ------------------------------------------------------------- mrank_finalize
// One block: strided chains, then a fixed LDS tree (cos_sum_kernel's shape).

__global__ __launch_bounds__(NT)
void mrank_finalize_kernel(const float* __restrict__ rho,
                           const float* __restrict__ dsum,
                           const int* __restrict__ old,
                           const float* __restrict__ sigma,
                           float* __restrict__ fin, int* __restrict__ nold,
                           int M, int k) {
  __shared__ float red_r[NT];
  __shared__ float red_d[NT];
  __shared__ int red_n[NT];
  float r = 0.f, d = 0.f;
  int n = 0;
  for (int i = threadIdx.x; i < M; i += NT) {
    r += rho[i];
    d += dsum[i];
    n += old[i];
  }
  red_r[threadIdx.x] = r;
  red_d[threadIdx.x] = d;
  red_n[threadIdx.x] = n;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red_r[threadIdx.x] += red_r[threadIdx.x + o];
      red_d[threadIdx.x] += red_d[threadIdx.x + o];
      red_n[threadIdx.x] += red_n[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float sg = sigma[0];
    const int N = red_n[0];
    nold[0] = N;
    if (sg > 0.f) {
      const float s = 1.f / sg;
      const float q = s / ((float)k * (float)(N > 1 ? N : 1));
      fin[0] = mr_mul_rn(q, red_r[0]);
      fin[1] = q;
      fin[2] = mr_mul_rn(mr_mul_rn(s, q), red_d[0]);
    } else {  // sigma <= 0 (or NaN): the loss and every gradient are 0
      fin[0] = 0.f;
      fin[1] = 0.f;
      fin[2] = 0.f;
    }
  }
}

// ------------------------------------------------------------------ mrank_bwd
// Writes the whole dlogits row: zeros plus the at most k + 1 entries.

__global__ __launch_bounds__(NT)
void mrank_bwd_kernel(const int* __restrict__ sel,
                      const long* __restrict__ targets,
                      const float* __restrict__ fin,
                      const float* __restrict__ up,
                      bf16_t* __restrict__ dlogits, float* __restrict__ dsig,
                      int M, int C, int known, int k) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * MR_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  const float u = up[0];
  if (row == 0 && lane == 0) dsig[0] = mr_mul_rn(u, fin[2]);
  const float gq = mr_mul_rn(u, fin[1]);
  const int* srow = sel + (long)row * k;
  int s[MR_KMAX];
  int A = 0;
#pragma unroll
  for (int j = 0; j < MR_KMAX; ++j) {
    s[j] = j < k ? srow[j] : -1;
    // an active pair names a new class; anything else writes nothing
    if (s[j] < known || s[j] >= C) s[j] = -1;
    A += s[j] >= 0 ? 1 : 0;
  }
  const long t = targets[row];
  const bf16_t pos = f2bf(gq);
  const bf16_t neg = f2bf(-mr_mul_rn(gq, (float)A));
  const bool has = A > 0 && t >= 0 && t < known;
  bf16_t* dr = dlogits + (long)row * C;
  for (int c = lane; c < C; c += WAVE) {
    bf16_t o = 0;
    if (has && c == (int)t) o = neg;
#pragma unroll
    for (int j = 0; j < MR_KMAX; ++j)
      if (c == s[j]) o = pos;
    dr[c] = o;
  }
}

static bool mrank_shape_ok(int M, int C, int known, int k) {
  return M >= 1 && C >= 2 && known >= 1 && known < C && k >= 1 &&
         k <= MR_KMAX && k <= C - known;
}

extern "C" {

// 1 when the launchers below accept the shape: M >= 1, C >= 2,
// 1 <= known < C, 1 <= k <= min(8, C - known)
int cilfw_mrank_supported(int M, int C, int known, int k) {
  return mrank_shape_ok(M, C, known, k) ? 1 : 0;
}

// logits bf16 (M, C), targets int64 (M), sigma fp32 (1) on the device ->
// rho, dsum fp32 (M), old int32 (M), sel int32 (M, k), fin fp32 (3) = {loss,
// q, dsigma for upstream 1}, nold int32 (1). Every element is written.
// Returns 0, or 1 when the arguments are refused (no launch).
int cilfw_mrank_fwd(const void* logits, const void* targets,
                    const void* sigma, void* rho, void* dsum, void* old,
                    void* sel, void* fin, void* nold, int M, int C, int known,
                    int k, float margin, void* stream) {
  if (!mrank_shape_ok(M, C, known, k) || !(margin >= 0.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mrank_fwd_kernel, dim3(cdiv(M, MR_ROWS)), dim3(NT), 0,
                     st, (const bf16_t*)logits, (const long*)targets,
                     (const float*)sigma, (float*)rho, (float*)dsum,
                     (int*)old, (int*)sel, M, C, known, k, margin);
  hipLaunchKernelGGL(mrank_finalize_kernel, dim3(1), dim3(NT), 0, st,
                     (const float*)rho, (const float*)dsum, (const int*)old,
                     (const float*)sigma, (float*)fin, (int*)nold, M, k);
  return 0;
}

// sel, targets, fin as written by cilfw_mrank_fwd; up: 1 fp32 on the device
// -> dlogits bf16 (M, C), dsig fp32 (1). Every element is written.
int cilfw_mrank_bwd(const void* sel, const void* targets, const void* fin,
                    const void* up, void* dlogits, void* dsig, int M, int C,
                    int known, int k, void* stream) {
  if (!mrank_shape_ok(M, C, known, k)) return 1;
  hipLaunchKernelGGL(mrank_bwd_kernel, dim3(cdiv(M, MR_ROWS)), dim3(NT), 0,
                     (hipStream_t)stream, (const int*)sel,
                     (const long*)targets, (const float*)fin,
                     (const float*)up, (bf16_t*)dlogits, (float*)dsig, M, C,
                     known, k);
  return 0;
}

}  // extern "C"
