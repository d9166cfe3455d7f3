// cilfw — nearest-mean-of-exemplars (NME) classifier kernels for gfx950.
//
// iCaRL's classification rule: a test feature goes to the class whose mean
// exemplar feature is nearest. With x^ = x / max(|x|, 1e-12):
//   prototype  p_c = m / max(|m|, 1e-12),  m = (1/q) sum_i f^_i
//   score      s(x, c) = x^ . p_c          (larger = nearer)
// Everything is exact fp32 with a fixed summation order: no float atomics,
// no split reductions whose order depends on the launch. Reruns are
// bit-identical (docs/kernels.md, "NME").

#include "common.h"

#define NT 256
#define NME_MAX_D 4096
#define NME_EPS 1e-12f

// fixed-order block sum: xor butterfly inside each wave, then the four wave
// partials added in wave order by every thread. red: NT / WAVE floats.
DEV float nme_block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------- prototypes
// One block per class. Thread t owns feature columns t, t+NT, ... (<= 16 of
// them, D <= 4096) in registers; the exemplars of the class are visited in
// row order, so column d of the mean is one sequential chain over the q
// exemplars and each norm is one nme_block_sum: the order depends on (q, D)
// only.

__global__ __launch_bounds__(NT)
void nme_proto_kernel(const float* __restrict__ feats,
                      const int* __restrict__ seg_off,
                      float* __restrict__ protos, int D) {
  constexpr int NJ = NME_MAX_D / NT;
  const int c = blockIdx.x;
  const int s = seg_off[c], e = seg_off[c + 1];
  __shared__ float red[NT / WAVE];
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  for (int i = s; i < e; ++i) {
    const float* fr = feats + (long)i * D;
    float v[NJ];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = threadIdx.x + j * NT;
      v[j] = d < D ? fr[d] : 0.f;
      ss = fmaf(v[j], v[j], ss);
    }
    ss = nme_block_sum(ss, red);
    const float inv = 1.f / fmaxf(sqrtf(ss), NME_EPS);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = fmaf(v[j], inv, acc[j]);
  }
  const int q = e - s;
  const float invq = q > 0 ? 1.f / (float)q : 0.f;  // wrapper refuses q == 0
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    acc[j] *= invq;
    ss = fmaf(acc[j], acc[j], ss);
  }
  ss = nme_block_sum(ss, red);
  const float inv = 1.f / fmaxf(sqrtf(ss), NME_EPS);
  float* pr = protos + (long)c * D;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = threadIdx.x + j * NT;
    if (d < D) pr[d] = acc[j] * inv;
  }
}

// ------------------------------------------------------------ fused top-k
// Block = 64 feature rows. Class tiles of 64 prototypes are visited in
// ascending order; for each, D is walked in tiles of 32 through LDS (both
// operands row-major, rows padded to 36 floats so the float4 fragment reads
// of 16 consecutive rows fall on distinct banks). Every prototype tile in LDS
// is used by all 64 rows of the block. Thread (ty, tx) holds the 4x4 scores
// of rows ty+16i and classes tx+16j; each is ONE fmaf chain over d = 0..D-1
// in ascending order (zero padding past D adds exact zeros), so the order is
// the same for every (row, class) wherever it sits in a tile: bitwise-equal
// prototypes score bitwise-equal. After a class tile the scaled scores go to
// LDS and one thread per row merges them, in ascending class order with a
// strict '>' insert, into its descending top-8 (one LDS column per row): ties
// keep the lower class index first. LDS and registers do not depend on N or C,
// and no (N, C) matrix ever reaches global memory.

// float4 q4 of row r of a (rows, 4*D4) matrix, zeros outside it. The load is
// unconditional from a clamped (always valid) address and the value selected
// afterwards: a select between two pointers would become a flat load.
DEV float4 nme_ld4(const float* __restrict__ base, int r, int rows, int D4,
                   int q4) {
  const bool ok = r < rows && q4 < D4;
  const long off = (long)min(r, rows - 1) * D4 + min(q4, D4 - 1);
  float4 v = ((const float4*)base)[off];
  v.x = ok ? v.x : 0.f;
  v.y = ok ? v.y : 0.f;
  v.z = ok ? v.z : 0.f;
  v.w = ok ? v.w : 0.f;
  return v;
}

#define NME_BM 64
#define NME_BN 64
#define NME_BK 32
#define NME_LDT (NME_BK + 4)
#define NME_LDS_S (NME_BN + 1)
#define NME_TOPK 8

__global__ __launch_bounds__(NT)
void nme_topk_kernel(const float* __restrict__ X, const float* __restrict__ P,
                     const long* __restrict__ targets,
                     int* __restrict__ idx_out, float* __restrict__ score_out,
                     unsigned long long* __restrict__ counts, int N, int C,
                     int D, int maxk) {
  __shared__ __attribute__((aligned(16))) float Xs[NME_BM * NME_LDT];
  __shared__ __attribute__((aligned(16))) float Ps[NME_BN * NME_LDT];
  __shared__ float Ss[NME_BM * NME_LDS_S];
  __shared__ float inv_s[NME_BM];
  __shared__ float top_s[NME_TOPK * NME_BM];  // [k][row], descending in k
  __shared__ int top_i[NME_TOPK * NME_BM];
  __shared__ int cnt_s[NME_TOPK];

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.x * NME_BM;
  const int D4 = D >> 2;

  // row norms: 4 lanes per row, each a strided chain, joined by a butterfly
  {
    const int r = tid >> 2, part = tid & 3;
    const int row = row0 + r;
    float ss = 0.f;
    if (row < N) {
      const float4* xr = (const float4*)(X + (long)row * D);
      for (int d4 = part; d4 < D4; d4 += 4) {
        const float4 v = xr[d4];
        ss = fmaf(v.x, v.x, ss);
        ss = fmaf(v.y, v.y, ss);
        ss = fmaf(v.z, v.z, ss);
        ss = fmaf(v.w, v.w, ss);
      }
    }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    if (part == 0) inv_s[r] = 1.f / fmaxf(sqrtf(ss), NME_EPS);
    if (tid < NME_TOPK) cnt_s[tid] = 0;
  }

  // running top-8 of row tid (threads 0..63): column tid of top_s / top_i,
  // touched by that thread alone; kth caches its smallest kept score
  float kth = -INFINITY;
  if (tid < NME_BM)
    for (int k = 0; k < NME_TOPK; ++k) {
      top_s[k * NME_BM + tid] = -INFINITY;
      top_i[k * NME_BM + tid] = -1;
    }

  // staging map: thread -> (row lr + 32h, float4 column lq) of a 64x32 tile
  const int lr = tid >> 3, lq = tid & 7;

  for (int c0 = 0; c0 < C; c0 += NME_BN) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float4 xg[2], pg[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      xg[h] = nme_ld4(X, row0 + lr + 32 * h, N, D4, lq);
      pg[h] = nme_ld4(P, c0 + lr + 32 * h, C, D4, lq);
    }

    for (int d0 = 0; d0 < D; d0 += NME_BK) {
      __syncthreads();  // the previous tile's reads (and the merge) are done
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = lr + 32 * h;
        *(float4*)&Xs[r * NME_LDT + lq * 4] = xg[h];
        *(float4*)&Ps[r * NME_LDT + lq * 4] = pg[h];
      }
      __syncthreads();
      if (d0 + NME_BK < D) {  // next tile's loads fly over this tile's FMAs
        const int q4 = ((d0 + NME_BK) >> 2) + lq;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          xg[h] = nme_ld4(X, row0 + lr + 32 * h, N, D4, q4);
          pg[h] = nme_ld4(P, c0 + lr + 32 * h, C, D4, q4);
        }
      }
#pragma unroll 2
      for (int k4 = 0; k4 < NME_BK / 4; ++k4) {
        float4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a[i] = *(const float4*)&Xs[(ty + 16 * i) * NME_LDT + k4 * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = *(const float4*)&Ps[(tx + 16 * j) * NME_LDT + k4 * 4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float s = acc[i][j];
            s = fmaf(a[i].x, b[j].x, s);
            s = fmaf(a[i].y, b[j].y, s);
            s = fmaf(a[i].z, b[j].z, s);
            s = fmaf(a[i].w, b[j].w, s);
            acc[i][j] = s;
          }
      }
    }

    // Ss was last read by the previous merge, which ended before the
    // barriers of the D loop above (D >= 4: at least one tile)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float inv = inv_s[ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        Ss[(ty + 16 * i) * NME_LDS_S + tx + 16 * j] = acc[i][j] * inv;
    }
    __syncthreads();
    if (tid < NME_BM) {
      const int nc = min(NME_BN, C - c0);
      for (int c = 0; c < nc; ++c) {
        const float v = Ss[tid * NME_LDS_S + c];
        if (v > kth) {
          int k = NME_TOPK - 1;
          // strict '>': an equal score of an earlier class stays in front
          while (k > 0 && v > top_s[(k - 1) * NME_BM + tid]) {
            top_s[k * NME_BM + tid] = top_s[(k - 1) * NME_BM + tid];
            top_i[k * NME_BM + tid] = top_i[(k - 1) * NME_BM + tid];
            --k;
          }
          top_s[k * NME_BM + tid] = v;
          top_i[k * NME_BM + tid] = c0 + c;
          kth = top_s[(NME_TOPK - 1) * NME_BM + tid];
        }
      }
    }
  }

  const int row = row0 + tid;
  if (tid < NME_BM && row < N) {
    int found = NME_TOPK;
    const int tgt = targets != nullptr ? (int)targets[row] : -2;
    for (int k = 0; k < maxk; ++k) {
      const int ci = top_i[k * NME_BM + tid];
      idx_out[(long)row * maxk + k] = ci;
      score_out[(long)row * maxk + k] = top_s[k * NME_BM + tid];
      if (ci == tgt && found == NME_TOPK) found = k;
    }
    if (counts != nullptr)
      for (int k = found; k < maxk; ++k) atomicAdd(&cnt_s[k], 1);
  }
  if (counts != nullptr) {  // uniform across the block
    __syncthreads();
    if (tid < maxk && cnt_s[tid] > 0)
      atomicAdd(&counts[tid], (unsigned long long)cnt_s[tid]);
  }
}

extern "C" {

// feats fp32 (n, D), rows grouped by class; seg_off int32 (C+1); protos fp32
// (C, D). D <= 4096.
void cilfw_nme_prototypes(const void* feats, const void* seg_off,
                          void* protos, int C, int D, void* stream) {
  if (C <= 0) return;
  hipLaunchKernelGGL(nme_proto_kernel, dim3(C), dim3(NT), 0,
                     (hipStream_t)stream, (const float*)feats,
                     (const int*)seg_off, (float*)protos, D);
}

// feats fp32 (N, D); protos fp32 (C, D); targets int64 (N) or null; idx int32
// (N, maxk); score fp32 (N, maxk); counts int64 (maxk) or null, zeroed here.
// D % 4 == 0, maxk <= min(8, C).
void cilfw_nme_topk(const void* feats, const void* protos,
                    const void* targets, void* idx, void* score, void* counts,
                    int N, int C, int D, int maxk, void* stream) {
  if (counts != nullptr)
    (void)hipMemsetAsync(counts, 0, maxk * sizeof(long), (hipStream_t)stream);
  if (N <= 0) return;
  hipLaunchKernelGGL(nme_topk_kernel, dim3(cdiv(N, NME_BM)), dim3(NT), 0,
                     (hipStream_t)stream, (const float*)feats,
                     (const float*)protos, (const long*)targets, (int*)idx,
                     (float*)score, (unsigned long long*)counts, N, C, D,
                     maxk);
}

}  // extern "C"
