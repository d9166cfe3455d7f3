// cilfw — k-means initialisation of the proxies of a multi-proxy cosine head
// (PODNet's LSC) for gfx950: seeding and every Lloyd iteration of every class
// in ONE launch, one block per class.
//
// Definition (docs/kernels.md, "k-means proxies"; ops/kmeans.py holds the same
// text), with x^ = x / max(|x|, 1e-12) and squared Euclidean distance on the
// unit rows of one class (n >= K rows):
//   seeding  centre 0 = the row nearest to the mean of the unit rows; centre j
//            = the row whose smallest distance to centres 0..j-1 is largest;
//            ties to the lower row index. Before the first pass only the K
//            seed rows are assigned, each to its own centre.
//   Lloyd    assign every row to its nearest centre (ties to the lower centre
//            index), then every centre with members becomes their mean, summed
//            in ascending row order; a centre without members keeps its value.
//            Stop after the first iteration whose assignment pass changed
//            nothing, or after max_iter; iters = assignment passes run.
//   output   centre / max(|centre|, 1e-12), class-local assign, iters.
//
// Summation orders, all fixed by (n, D) alone (no float atomics; reruns are
// bit-identical, and a class gives the same bits alone or in a batch):
//   * every D-term sum (row norm, |x^|^2, |c_k|^2, x^ . c_k) is km_dot4's:
//     lane l of a wave chains the float4s l, l + 64, ... of the row with fmaf
//     in x, y, z, w order, then one xor butterfly 32, 16, ..., 1;
//   * column d of a mean is one sequential chain over the member rows in
//     ascending row order, then one division by the count.
// A seed centre is a bit copy of its row, so its |c|^2 and x^ . c carry the
// bits of the row's |x^|^2 and its distance to itself is exactly 0.

#include "common.h"

#define NT 256
#define KM_NW (NT / WAVE)
#define KM_MAX_K 16
#define KM_MAX_D 4096
#define KM_MAX_KD 16000
#define KM_EPS 1e-12f
// LDS after the (K, D) centres: c2[16], cnt[16], seed[16], redv[4], redi[4],
// flag
#define KM_LDS_TAIL (3 * KM_MAX_K + 2 * KM_NW + 4)

DEV float km_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum_d a[d] b[d] over D4 float4s in the fixed lane order; every lane returns
// the sum.
DEV float km_dot4(const float4* a, const float4* b, int D4) {
  float p = 0.f;
  for (int q = threadIdx.x & 63; q < D4; q += WAVE) {
    const float4 u = a[q], v = b[q];
    p = fmaf(u.x, v.x, p);
    p = fmaf(u.y, v.y, p);
    p = fmaf(u.z, v.z, p);
    p = fmaf(u.w, v.w, p);
  }
  return km_wave_sum(p);
}

// Values another thread of the block wrote earlier in this launch: read them
// with a relaxed workgroup-scope atomic load, which is never turned into a
// scalar (constant-cache) load.
DEV float km_ldf(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
DEV int km_ldi(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// global writes of the block become visible to the block
DEV void km_sync() {
  __threadfence_block();
  __syncthreads();
}

// Row index in [0, n) with the largest sgn * dmin; ties to the lower index.
// Block-uniform result. (val, idx) pairs are totally ordered, so the result
// does not depend on the order of the merges.
DEV int km_argbest(const float* dmin, int n, float sgn, float* redv,
                   int* redi) {
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += NT) {
    const float v = sgn * km_ldf(dmin + i);
    if (v > bv) { bv = v; bi = i; }  // ascending i: the lower index stays
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  __syncthreads();  // the previous use of redv / redi is over
  if ((threadIdx.x & 63) == 0) {
    redv[threadIdx.x >> 6] = bv;
    redi[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = redv[0];
  bi = redi[0];
#pragma unroll
  for (int w = 1; w < KM_NW; ++w) {
    const float ov = redv[w];
    const int oi = redi[w];
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  return min(bi, n - 1);  // finite features (the wrapper's check): a row won
}

// Squared distance of every row of the class to the vector in LDS slot j:
// dmin[i] = d (first) or min(dmin[i], d). Row i is always handled by wave
// i % 4, so the read-modify-write of dmin[i] stays inside one wave.
DEV void km_dist_pass(const float* xh, const float* xx, float* dmin,
                      const float* cen, const float* c2, int j, int n, int D,
                      bool first) {
  const int D4 = D >> 2;
  const float cc = c2[j];
  for (int i = threadIdx.x >> 6; i < n; i += KM_NW) {
    const float dot = km_dot4((const float4*)(xh + (long)i * D),
                              (const float4*)(cen + j * D), D4);
    if ((threadIdx.x & 63) == 0) {
      float d = fmaxf(fmaf(-2.f, dot, cc) + km_ldf(xx + i), 0.f);
      if (!first) d = fminf(km_ldf(dmin + i), d);
      dmin[i] = d;
    }
  }
}

// |c_j|^2 of the vector in LDS slot j, by wave 0.
DEV void km_c2(const float* cen, float* c2, int j, int D) {
  if (threadIdx.x < WAVE) {
    const float4* cj = (const float4*)(cen + j * D);
    const float v = km_dot4(cj, cj, D >> 2);
    if (threadIdx.x == 0) c2[j] = v;
  }
}

// KB: the compiled number of dot-product accumulators, K <= KB.
template <int KB>
__global__ __launch_bounds__(NT)
void kmeans_proxy_kernel(const float* __restrict__ feats,
                         const int* __restrict__ seg_off, float* xh, float* xx,
                         float* dmin, float* __restrict__ proxies, int* assign,
                         int* __restrict__ iters, int D, int K, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) float km_sh[];
  float* cen = km_sh;                     // (K, D) centres
  float* c2 = km_sh + K * D;              // |c_k|^2
  int* cnt = (int*)(c2 + KM_MAX_K);       // members of centre k
  int* seed = cnt + KM_MAX_K;             // seed rows
  float* redv = (float*)(seed + KM_MAX_K);
  int* redi = (int*)(redv + KM_NW);
  int* flag = redi + KM_NW;

  const int c = blockIdx.x;
  const int s = seg_off[c], n = seg_off[c + 1] - s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D4 = D >> 2;
  // this class's slices of the per-row buffers
  feats += (long)s * D;
  xh += (long)s * D;
  xx += s;
  dmin += s;
  assign += s;

  // ---- unit rows and their squared norms; nothing is assigned yet
  for (int i = tid; i < n; i += NT) assign[i] = -1;
  for (int i = wave; i < n; i += KM_NW) {
    const float4* fr = (const float4*)(feats + (long)i * D);
    float4* xr = (float4*)(xh + (long)i * D);
    const float ss = km_dot4(fr, fr, D4);
    const float inv = 1.f / fmaxf(sqrtf(ss), KM_EPS);
    float p = 0.f;
    for (int q = lane; q < D4; q += WAVE) {
      float4 v = fr[q];
      v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
      xr[q] = v;
      p = fmaf(v.x, v.x, p);
      p = fmaf(v.y, v.y, p);
      p = fmaf(v.z, v.z, p);
      p = fmaf(v.w, v.w, p);
    }
    p = km_wave_sum(p);
    if (lane == 0) xx[i] = p;
  }
  km_sync();

  // ---- seeding: the mean of the unit rows goes to slot 0 first
  for (int d = tid; d < D; d += NT) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += xh[(long)i * D + d];
    cen[d] = acc / (float)n;
  }
  __syncthreads();
  km_c2(cen, c2, 0, D);
  __syncthreads();
  km_dist_pass(xh, xx, dmin, cen, c2, 0, n, D, true);
  km_sync();
  int row = km_argbest(dmin, n, -1.f, redv, redi);  // nearest to the mean
  for (int j = 0; j < K; ++j) {
    // every read of slot j's previous content (the mean) is behind the
    // barriers of km_argbest
    for (int d = tid; d < D; d += NT) cen[j * D + d] = xh[(long)row * D + d];
    if (tid == 0) {
      seed[j] = row;
      assign[row] = j;  // ascending j in one thread
    }
    __syncthreads();
    km_c2(cen, c2, j, D);
    __syncthreads();
    if (j + 1 < K) {
      km_dist_pass(xh, xx, dmin, cen, c2, j, n, D, j == 0);
      km_sync();
      row = km_argbest(dmin, n, 1.f, redv, redi);  // farthest from its centre
    }
  }
  km_sync();

  // ---- Lloyd iterations
  int it = 0;
  while (it < max_iter) {
    ++it;
    if (tid < KM_MAX_K) cnt[tid] = 0;
    if (tid == 0) *flag = 0;
    __syncthreads();
    // assignment: wave w takes rows w, w + 4, ...; K dot products per lane
    for (int i = wave; i < n; i += KM_NW) {
      const float4* xr = (const float4*)(xh + (long)i * D);
      float acc[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) acc[k] = 0.f;
      for (int q = lane; q < D4; q += WAVE) {
        const float4 u = xr[q];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          // slots past K read slot K - 1: valid LDS, result unused
          const float4 v = ((const float4*)(cen + min(k, K - 1) * D))[q];
          float p = acc[k];
          p = fmaf(u.x, v.x, p);
          p = fmaf(u.y, v.y, p);
          p = fmaf(u.z, v.z, p);
          p = fmaf(u.w, v.w, p);
          acc[k] = p;
        }
      }
#pragma unroll
      for (int k = 0; k < KB; ++k) acc[k] = km_wave_sum(acc[k]);
      if (lane == 0) {
        const float xi = km_ldf(xx + i);
        int best = 0;
        float bd = fmaxf(fmaf(-2.f, acc[0], c2[0]) + xi, 0.f);
#pragma unroll
        for (int k = 1; k < KB; ++k) {
          const float d = fmaxf(fmaf(-2.f, acc[k], c2[min(k, K - 1)]) + xi,
                                0.f);
          if (k < K && d < bd) { bd = d; best = k; }  // strict: lower k stays
        }
        if (best != km_ldi(assign + i)) {
          assign[i] = best;
          *flag = 1;
        }
        atomicAdd(&cnt[best], 1);  // integer: order-free
      }
    }
    km_sync();
    const int changed = *flag;
    // update: thread t owns columns t, t + 256, ... of every centre
    for (int d = tid; d < D; d += NT) {
      for (int k = 0; k < K; ++k)
        if (cnt[k] > 0) cen[k * D + d] = 0.f;
      int i = 0;
      for (; i + 4 <= n; i += 4) {  // loads of four rows fly together
        int a[4];
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a[r] = km_ldi(assign + i + r);
          v[r] = xh[(long)(i + r) * D + d];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) cen[a[r] * D + d] += v[r];
      }
      for (; i < n; ++i)
        cen[km_ldi(assign + i) * D + d] += xh[(long)i * D + d];
      for (int k = 0; k < K; ++k)
        if (cnt[k] > 0) cen[k * D + d] /= (float)cnt[k];
    }
    __syncthreads();
    for (int k = wave; k < K; k += KM_NW) {
      const float4* ck = (const float4*)(cen + k * D);
      const float v = km_dot4(ck, ck, D4);
      if (lane == 0) c2[k] = v;
    }
    __syncthreads();  // also: every read of flag and cnt is over
    if (!changed) break;
  }

  if (tid == 0) iters[c] = it;
  for (int k = 0; k < K; ++k) {
    const float inv = 1.f / fmaxf(sqrtf(c2[k]), KM_EPS);
    float* pr = proxies + ((long)c * K + k) * D;
    for (int d = tid; d < D; d += NT) pr[d] = cen[k * D + d] * inv;
  }
}

extern "C" {

// 1 if one block can run classes of which the smallest has n rows: the (K, D)
// centres fit the LDS budget and every class has a row per centre.
int cilfw_kmeans_supported(int n, int D, int K) {
  if (D % 4 != 0 || D < 4 || D > KM_MAX_D) return 0;
  if (K < 1 || K > KM_MAX_K) return 0;
  if ((long)K * D > KM_MAX_KD) return 0;
  if (n < K) return 0;
  return 1;
}

// feats fp32 (n, D), rows grouped by class; seg_off int32 (C+1), every class
// with >= K rows (checked by the caller on the host); xh fp32 (n, D), xx and
// dmin fp32 (n) scratch; proxies fp32 (C*K, D); assign int32 (n); iters int32
// (C). Returns 1 (nothing launched) if the shape is refused.
int cilfw_kmeans_proxies(const void* feats, const void* seg_off, void* xh,
                         void* xx, void* dmin, void* proxies, void* assign,
                         void* iters, int C, int n_min, int D, int K,
                         int max_iter, void* stream) {
  if (C <= 0 || max_iter < 1 || !cilfw_kmeans_supported(n_min, D, K)) return 1;
  const size_t shmem = ((size_t)K * D + KM_LDS_TAIL) * sizeof(float);
#define KM_LAUNCH(KB)                                                        \
  hipLaunchKernelGGL(kmeans_proxy_kernel<KB>, dim3(C), dim3(NT), shmem,      \
                     (hipStream_t)stream, (const float*)feats,               \
                     (const int*)seg_off, (float*)xh, (float*)xx,            \
                     (float*)dmin, (float*)proxies, (int*)assign,            \
                     (int*)iters, D, K, max_iter)
  if (K <= 4) KM_LAUNCH(4);
  else if (K <= 8) KM_LAUNCH(8);
  else KM_LAUNCH(16);
#undef KM_LAUNCH
  return 0;
}

}  // extern "C"
