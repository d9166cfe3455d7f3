// cilfw — pooled-outputs distillation (PODNet's POD-spatial) for gfx950.
//
// One stage, student map a and teacher map b, both (N, H, W, C) bf16 NHWC:
//   pooled  v(a)_n = [ r | q ],  r[h,c] = sum_w a[n,h,w,c]^2,
//                                q[w,c] = sum_h a[n,h,w,c]^2     (N, H+W, C) fp32
//   v^ = v / max(|v|, 1e-12),  d_n = |v^(a)_n - v^(b)_n|,  loss = mean_n d_n
//   u = v^_s - v^_t,  g^ = u / (N d)  (0 when d == 0),
//   g_v = (g^ - v^_s (v^_s . g^)) / max(|v_s|, 1e-12)
//   da[n,h,w,c] = 2 a[n,h,w,c] (g_v.r[h,c] + g_v.q[w,c]) * upstream
// bf16 in, fp32 accumulate, no atomics; every sum has an order fixed by the
// shape alone, so two launches are bit-identical (docs/kernels.md, "POD").

#include "common.h"

#define NT 256
#define POD_EPS 1e-12f
#define POD_MAX_HW 256
#define POD_MAX_KJ 8          // 16-byte items of one row slab per lane
#define POD_MAX_ITEMS (WAVE * POD_MAX_KJ)

// ------------------------------------------------------------------ pod_pool
// Block = (sample n, slab of GB channel groups); a channel group is 8
// channels = one 16-byte load. GB is a power of two <= 64 with W * GB <=
// 512, so one row of the slab is at most 512 items, item j = w * GB + gl,
// and lane l of a wave holds items l, l + 64, ...: consecutive lanes read
// consecutive 16-byte pieces of a GB * 16-byte run per pixel (the whole
// pixel when GB covers C). Because GB divides 64, all items of a lane share
// one channel group gl = l % GB.
//   The four waves split the rows: wave v walks h = v, v + 4, ... Row sum
// r[h, gl]: the lane's items in ascending w, then an xor butterfly over the
// lanes that share gl; written straight to global. Column sums q: each lane
// keeps one fp32 x 8 accumulator per item across its rows (ascending h); at
// the end waves 1..3 park theirs in LDS and wave 0 adds them in wave order.

template <int KJ>
__global__ __launch_bounds__(NT)
void pod_pool_kernel(const bf16_t* __restrict__ a, float* __restrict__ out,
                     int H, int W, int C, int GB, int lgGB) {
  __shared__ __attribute__((aligned(16))) float qs[3 * KJ * WAVE * 8];
  const int n = blockIdx.x, g0 = blockIdx.y * GB;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = lane & (GB - 1);
  const int C8 = C >> 3;
  const bool gok = g0 + gl < C8;
  const int J = W << lgGB;  // items per row of the slab
  const bf16_t* an = a + (long)n * H * W * C + (long)(g0 + gl) * 8;
  float* on = out + (long)n * (H + W) * C + (long)(g0 + gl) * 8;

  float q[KJ][8];
#pragma unroll
  for (int k = 0; k < KJ; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) q[k][e] = 0.f;

  for (int h = wv; h < H; h += 4) {
    const bf16_t* ar = an + (long)h * W * C;
    bf16x8 v[KJ];
#pragma unroll
    for (int k = 0; k < KJ; ++k) {
      const int j = lane + k * WAVE;
      const int w = j >> lgGB;
      v[k] = (bf16x8)(short)0;
      if (gok && j < J) v[k] = *(const bf16x8*)(ar + (long)w * C);
    }
    float r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = 0.f;
#pragma unroll
    for (int k = 0; k < KJ; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = bf2f((bf16_t)v[k][e]);
        const float s = x * x;  // exact in fp32: 8-bit significands
        q[k][e] += s;
        r[e] += s;
      }
    for (int o = GB; o < WAVE; o <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] += __shfl_xor(r[e], o);
    if (lane < GB && gok) {
      float4* dst = (float4*)(on + (long)h * C);
      dst[0] = make_float4(r[0], r[1], r[2], r[3]);
      dst[1] = make_float4(r[4], r[5], r[6], r[7]);
    }
  }

  if (wv > 0) {
#pragma unroll
    for (int k = 0; k < KJ; ++k) {
      float4* dst = (float4*)&qs[(((wv - 1) * KJ + k) * WAVE + lane) * 8];
      dst[0] = make_float4(q[k][0], q[k][1], q[k][2], q[k][3]);
      dst[1] = make_float4(q[k][4], q[k][5], q[k][6], q[k][7]);
    }
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int k = 0; k < KJ; ++k) {
      const int j = lane + k * WAVE;
      const int w = j >> lgGB;
      for (int p = 0; p < 3; ++p) {
        const float* src = &qs[((p * KJ + k) * WAVE + lane) * 8];
#pragma unroll
        for (int e = 0; e < 8; ++e) q[k][e] += src[e];
      }
      if (gok && j < J) {
        float4* dst = (float4*)(on + (long)(H + w) * C);
        dst[0] = make_float4(q[k][0], q[k][1], q[k][2], q[k][3]);
        dst[1] = make_float4(q[k][4], q[k][5], q[k][6], q[k][7]);
      }
    }
  }
}

// fixed-order block sums of two values at once: xor butterfly inside each
// wave, then the four wave partials added in wave order by every thread.
// red: 2 * NT / WAVE floats.
DEV void pod_block_sum2(float& x, float& y, float* red) {
  for (int o = 32; o > 0; o >>= 1) {
    x += __shfl_xor(x, o);
    y += __shfl_xor(y, o);
  }
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = x;
    red[4 + (threadIdx.x >> 6)] = y;
  }
  __syncthreads();
  x = ((red[0] + red[1]) + red[2]) + red[3];
  y = ((red[4] + red[5]) + red[6]) + red[7];
}

// v^_s element (sh) and u = v^_s - v^_t. The products are rounded on their
// own (no contraction into an fma), so bitwise-equal inputs give u == 0.
DEV float pod_u(float s, float t, float is, float it, float& sh) {
#pragma clang fp contract(off)
  sh = s * is;
  const float th = t * it;
  return sh - th;
}

// ------------------------------------------------------------------ pod_dist
// One block per sample over the two pooled vectors (length L = (H+W) C, a
// multiple of 8; they were just written and sit in L2, so the three passes
// re-read them from there). Thread t owns float4 t, t + NT, ... in every
// pass, so each block sum has the same order on every launch.

__global__ __launch_bounds__(NT)
void pod_dist_kernel(const float* __restrict__ vs, const float* __restrict__ vt,
                     float* __restrict__ gv, float* __restrict__ dist, int L,
                     float invN) {
  __shared__ float red[2 * NT / WAVE];
  const int n = blockIdx.x;
  const int L4 = L >> 2;
  const float4* s4 = (const float4*)(vs + (long)n * L);
  const float4* t4 = (const float4*)(vt + (long)n * L);
  float4* g4 = (float4*)(gv + (long)n * L);

  float ss = 0.f, tt = 0.f;
  for (int i = threadIdx.x; i < L4; i += NT) {
    const float4 s = s4[i], t = t4[i];
    ss = fmaf(s.x, s.x, ss); ss = fmaf(s.y, s.y, ss);
    ss = fmaf(s.z, s.z, ss); ss = fmaf(s.w, s.w, ss);
    tt = fmaf(t.x, t.x, tt); tt = fmaf(t.y, t.y, tt);
    tt = fmaf(t.z, t.z, tt); tt = fmaf(t.w, t.w, tt);
  }
  pod_block_sum2(ss, tt, red);
  const float is = 1.f / fmaxf(sqrtf(ss), POD_EPS);
  const float it = 1.f / fmaxf(sqrtf(tt), POD_EPS);

  // d^2 = sum u^2 and p = v^_s . u
  float dd = 0.f, p = 0.f;
  for (int i = threadIdx.x; i < L4; i += NT) {
    const float4 s = s4[i], t = t4[i];
    float sh, u;
    u = pod_u(s.x, t.x, is, it, sh); dd = fmaf(u, u, dd); p = fmaf(sh, u, p);
    u = pod_u(s.y, t.y, is, it, sh); dd = fmaf(u, u, dd); p = fmaf(sh, u, p);
    u = pod_u(s.z, t.z, is, it, sh); dd = fmaf(u, u, dd); p = fmaf(sh, u, p);
    u = pod_u(s.w, t.w, is, it, sh); dd = fmaf(u, u, dd); p = fmaf(sh, u, p);
  }
  pod_block_sum2(dd, p, red);
  const float d = sqrtf(dd);
  if (threadIdx.x == 0) dist[n] = d;
  // g^ = k u with k = 1 / (N d), exactly 0 at d == 0;
  // g_v = (g^ - v^_s (v^_s . g^)) / |v_s| = k (u - v^_s p) / |v_s|
  const float k = d > 0.f ? invN / d : 0.f;
  const float kk = k * is;
  for (int i = threadIdx.x; i < L4; i += NT) {
    const float4 s = s4[i], t = t4[i];
    float4 g;
    float sh, u;
    u = pod_u(s.x, t.x, is, it, sh); g.x = kk * (u - sh * p);
    u = pod_u(s.y, t.y, is, it, sh); g.y = kk * (u - sh * p);
    u = pod_u(s.z, t.z, is, it, sh); g.z = kk * (u - sh * p);
    u = pod_u(s.w, t.w, is, it, sh); g.w = kk * (u - sh * p);
    g4[i] = g;
  }
}

// loss = scale * sum_n dist[n]: strided chains, then a fixed LDS tree (the
// shape of loss.hip's loss_mean_kernel). One block.
__global__ __launch_bounds__(NT)
void pod_mean_kernel(const float* __restrict__ dist, float* __restrict__ loss,
                     int N, float scale) {
  __shared__ float red[NT];
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += NT) s += dist[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] * scale;
}

// ------------------------------------------------------------------- pod_bwd
// One thread per 16-byte item of a: 16 bytes of a in, two 32-byte pieces of
// g_v (L2-resident: g_v is (H+W)/(2 H W) the size of a) and 16 bytes of da
// out. Consecutive threads walk consecutive items of the flat map.

__global__ __launch_bounds__(NT)
void pod_bwd_kernel(const bf16_t* __restrict__ a, const float* __restrict__ gv,
                    const float* __restrict__ up, bf16_t* __restrict__ da,
                    long items, int H, int W, int C8) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= items) return;
  const int g = (int)(i % C8);
  const long pix = i / C8;
  const int w = (int)(pix % W);
  const long nh = pix / W;
  const int h = (int)(nh % H);
  const long n = nh / H;
  const int C = C8 * 8;
  const float* gn = gv + n * (long)(H + W) * C + g * 8;
  const float4* gr = (const float4*)(gn + (long)h * C);
  const float4* gq = (const float4*)(gn + (long)(H + w) * C);
  const float4 r0 = gr[0], r1 = gr[1], q0 = gq[0], q1 = gq[1];
  const float t[8] = {r0.x + q0.x, r0.y + q0.y, r0.z + q0.z, r0.w + q0.w,
                      r1.x + q1.x, r1.y + q1.y, r1.z + q1.z, r1.w + q1.w};
  const float s = 2.f * up[0];
  const bf16x8 v = *(const bf16x8*)(a + i * 8);
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    o[e] = (short)f2bf(s * bf2f((bf16_t)v[e]) * t[e]);
  *(bf16x8*)(da + i * 8) = o;
}

static bool pod_shape_ok(int N, int H, int W, int C) {
  return N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && H <= POD_MAX_HW &&
         W <= POD_MAX_HW;
}

extern "C" {

// 1 when the launchers below accept the shape (C % 8 == 0, H, W <= 256)
int cilfw_pod_supported(int N, int H, int W, int C) {
  return pod_shape_ok(N, H, W, C) ? 1 : 0;
}

// channel groups per pod_pool block for a map of width W with C channels
int cilfw_pod_pool_groups(int W, int C) {
  int gb = 1;
  while (gb * 2 <= WAVE && gb * 2 * W <= POD_MAX_ITEMS && gb < C / 8) gb *= 2;
  return gb;
}

// a bf16 (N, H, W, C) -> out fp32 (N, H+W, C), every element written.
// Returns 0, or 1 when the shape is refused (nothing is launched).
int cilfw_pod_pool(const void* a, void* out, int N, int H, int W, int C,
                   void* stream) {
  if (!pod_shape_ok(N, H, W, C)) return 1;
  const int gb = cilfw_pod_pool_groups(W, C);
  int lg = 0;
  while ((1 << lg) < gb) ++lg;
  const int kj = cdiv(W * gb, WAVE);
  const dim3 grid(N, cdiv(C / 8, gb));
  hipStream_t st = (hipStream_t)stream;
#define POD_POOL_LAUNCH(KJ)                                              \
  hipLaunchKernelGGL(pod_pool_kernel<KJ>, grid, dim3(NT), 0, st,         \
                     (const bf16_t*)a, (float*)out, H, W, C, gb, lg)
  if (kj <= 1) POD_POOL_LAUNCH(1);
  else if (kj <= 2) POD_POOL_LAUNCH(2);
  else if (kj <= 4) POD_POOL_LAUNCH(4);
  else POD_POOL_LAUNCH(8);
#undef POD_POOL_LAUNCH
  return 0;
}

// vs, vt fp32 (N, L) pooled vectors, L % 8 == 0 -> gv fp32 (N, L) for
// upstream 1, dist fp32 (N), loss fp32 (1) = mean_n dist.
int cilfw_pod_dist(const void* vs, const void* vt, void* gv, void* dist,
                   void* loss, int N, int L, void* stream) {
  if (N <= 0 || L <= 0 || L % 8 != 0) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pod_dist_kernel, dim3(N), dim3(NT), 0, st,
                     (const float*)vs, (const float*)vt, (float*)gv,
                     (float*)dist, L, 1.f / (float)N);
  hipLaunchKernelGGL(pod_mean_kernel, dim3(1), dim3(NT), 0, st,
                     (const float*)dist, (float*)loss, N, 1.f / (float)N);
  return 0;
}

// da bf16 (N, H, W, C) = 2 a (gv.r[h] + gv.q[w]) * up[0]; up: 1 fp32 on the
// device. Every element of da is written.
int cilfw_pod_bwd(const void* a, const void* gv, const void* up, void* da,
                  int N, int H, int W, int C, void* stream) {
  if (!pod_shape_ok(N, H, W, C)) return 1;
  const long items = (long)N * H * W * (C / 8);
  const long blocks = (items + NT - 1) / NT;
  if (blocks > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(pod_bwd_kernel, dim3((unsigned)blocks), dim3(NT), 0,
                     (hipStream_t)stream, (const bf16_t*)a, (const float*)gv,
                     (const float*)up, (bf16_t*)da, items, H, W, C / 8);
  return 0;
}

}  // extern "C"
