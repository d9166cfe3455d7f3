// cilfw — row-wise L2 normalisation family for gfx950: the cosine classifier
// head (LUCIR / PODNet's one-proxy LSC) and the embedding distillation
// ("less-forget" / POD-flat).
//
// Inverse norm of a row x of length D: r(x) = 1/|x| if |x| > 0, else 0 (a
// zero row gives a zero unit vector and an exactly zero gradient, never
// 1/eps).
//   rownorm_fwd   y = bf16(s * (x r(x))), rinv = r(x); s = scale[0] read on
//                 the device, or 1 without a scale pointer
//   rownorm_bwd   dx = (s r) (G - x^ (x^ . G)), x^ = x r; dsig[row] = x^ . G
//   flat_dist     u = s^ - t^, l = |u|^2 / 2, gs = (1/M) r(s) (u - s^ (s^.u))
//   flat_bwd      ds = bf16(up[0] * gs)
//   cos_sum       out[0] = scale * sum_i v[i], one block, fixed order
// The (M, C) products of the head go through the GEMMs of gemm.hip on the
// normalised operands (docs/kernels.md, "Cosine head / flat").
//
// One wave per row, four rows per 256-thread block: the row sums are an xor
// butterfly inside the wave, so there is no LDS and no block barrier. A row
// (D <= 2048) lives in registers: lane l holds the 16-byte items l, l + 64,
// ... (8 bf16 or 4 fp32 values each, at most 32 values per lane). fp32
// accumulate, no atomics; every sum has an order fixed by the shape alone, so
// two launches are bit-identical.

#include "common.h"

#define NT 256
#define COS_MAX_D 2048
#define COS_ROWS (NT / WAVE)

typedef __attribute__((ext_vector_type(4))) short bf16x4;

// Row<F32>: VEC values per 16-byte item, KMAX items per lane at D = 2048.
template <bool F32> struct Row;
template <> struct Row<false> {
  static constexpr int VEC = 8, KMAX = COS_MAX_D / (8 * WAVE);
  typedef bf16_t elem;
  static DEV void load(const elem* p, float* v) {
    const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bf2f((bf16_t)t[e]);
  }
  static DEV void store(elem* p, const float* v) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (short)f2bf(v[e]);
    *(bf16x8*)p = t;
  }
};
template <> struct Row<true> {
  static constexpr int VEC = 4, KMAX = COS_MAX_D / (4 * WAVE);
  typedef float elem;
  static DEV void load(const elem* p, float* v) {
    const float4 t = *(const float4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static DEV void store(elem* p, const float* v) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  }
};

DEV float wave_sum(float x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

DEV float inv_norm(float ss) {
  const float n = sqrtf(ss);
  return n > 0.f ? 1.f / n : 0.f;
}

// a * b rounded on its own: the caller's add or subtract never contracts
// with it into an fma
DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

// --------------------------------------------------------------- rownorm_fwd
// y is bf16 whatever the input type: it is the GEMM operand.

template <bool F32>
__global__ __launch_bounds__(NT)
void rownorm_fwd_kernel(const typename Row<F32>::elem* __restrict__ x,
                        const float* __restrict__ scale,
                        bf16_t* __restrict__ y, float* __restrict__ rinv,
                        int rows, int D) {
  typedef Row<F32> R;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * COS_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole waves leave; there is no barrier below
  const int items = D / R::VEC;
  const typename R::elem* xr = x + (long)row * D;
  bf16_t* yr = y + (long)row * D;

  float v[R::KMAX][R::VEC];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
#pragma unroll
    for (int e = 0; e < R::VEC; ++e) v[k][e] = 0.f;
    if (j < items) R::load(xr + j * R::VEC, v[k]);
#pragma unroll
    for (int e = 0; e < R::VEC; ++e) ss = fmaf(v[k][e], v[k][e], ss);
  }
  const float r = inv_norm(wave_sum(ss));
  const float s = scale ? scale[0] : 1.f;
  if (lane == 0) rinv[row] = r;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
    if (j < items) {
      if (R::VEC == 8) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          o[e] = (short)f2bf(mul_rn(s, mul_rn(v[k][e], r)));
        *(bf16x8*)(yr + j * 8) = o;
      } else {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = (short)f2bf(mul_rn(s, mul_rn(v[k][e], r)));
        *(bf16x4*)(yr + j * 4) = o;
      }
    }
  }
}

// --------------------------------------------------------------- rownorm_bwd
// x, G and dx share one type: bf16 for features, fp32 for class weights.

template <bool F32>
__global__ __launch_bounds__(NT)
void rownorm_bwd_kernel(const typename Row<F32>::elem* __restrict__ x,
                        const float* __restrict__ rinv,
                        const typename Row<F32>::elem* __restrict__ G,
                        const float* __restrict__ scale,
                        typename Row<F32>::elem* __restrict__ dx,
                        float* __restrict__ dsig, int rows, int D) {
  typedef Row<F32> R;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * COS_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int items = D / R::VEC;
  const long base = (long)row * D;
  const float r = rinv[row];

  float xh[R::KMAX][R::VEC], g[R::KMAX][R::VEC];
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
#pragma unroll
    for (int e = 0; e < R::VEC; ++e) xh[k][e] = g[k][e] = 0.f;
    if (j < items) {
      R::load(x + base + j * R::VEC, xh[k]);
      R::load(G + base + j * R::VEC, g[k]);
    }
#pragma unroll
    for (int e = 0; e < R::VEC; ++e) {
      xh[k][e] = mul_rn(xh[k][e], r);
      p = fmaf(xh[k][e], g[k][e], p);
    }
  }
  p = wave_sum(p);
  if (dsig && lane == 0) dsig[row] = p;
  // r == 0 (zero row): x^ == 0, p == 0 and sr == 0, so dx == 0 exactly
  const float sr = (scale ? scale[0] : 1.f) * r;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
    if (j < items) {
      float o[R::VEC];
#pragma unroll
      for (int e = 0; e < R::VEC; ++e)
        o[e] = sr * (g[k][e] - mul_rn(xh[k][e], p));
      R::store(dx + base + j * R::VEC, o);
    }
  }
}

// ----------------------------------------------------------------- flat_dist
// Student s and teacher t rows, bf16. One pass over both: the rows stay in
// registers between the norms, the distance and the saved gradient.

__global__ __launch_bounds__(NT)
void flat_dist_kernel(const bf16_t* __restrict__ s, const bf16_t* __restrict__ t,
                      float* __restrict__ gs, float* __restrict__ l, int rows,
                      int D, float invM) {
  typedef Row<false> R;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * COS_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int items = D / 8;
  const long base = (long)row * D;

  float a[R::KMAX][8], b[R::KMAX][8];
  float ss = 0.f, tt = 0.f;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[k][e] = b[k][e] = 0.f;
    if (j < items) {
      R::load(s + base + j * 8, a[k]);
      R::load(t + base + j * 8, b[k]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ss = fmaf(a[k][e], a[k][e], ss);
      tt = fmaf(b[k][e], b[k][e], tt);
    }
  }
  const float rs = inv_norm(wave_sum(ss));
  const float rt = inv_norm(wave_sum(tt));

  // a <- s^, b <- u = s^ - t^: the two products are rounded on their own, so
  // bitwise-equal rows give u == 0
  float dd = 0.f, p = 0.f;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a[k][e] = mul_rn(a[k][e], rs);
      b[k][e] = a[k][e] - mul_rn(b[k][e], rt);
      dd = fmaf(b[k][e], b[k][e], dd);
      p = fmaf(a[k][e], b[k][e], p);
    }
  dd = wave_sum(dd);
  p = wave_sum(p);
  if (lane == 0) l[row] = 0.5f * dd;
  const float kk = invM * rs;
#pragma unroll
  for (int k = 0; k < R::KMAX; ++k) {
    const int j = lane + k * WAVE;
    if (j < items) {
      float4* dst = (float4*)(gs + base + j * 8);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[e] = kk * (b[k][e] - mul_rn(a[k][e], p));
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
  }
}

// ds = bf16(up[0] * gs), one thread per 8 values
__global__ __launch_bounds__(NT)
void flat_bwd_kernel(const float* __restrict__ gs, const float* __restrict__ up,
                     bf16_t* __restrict__ ds, long items) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= items) return;
  const float4* src = (const float4*)(gs + i * 8);
  const float4 g0 = src[0], g1 = src[1];
  const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  const float u = up[0];
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(u * g[e]);
  *(bf16x8*)(ds + i * 8) = o;
}

// out[0] = scale * sum_i v[i]: strided chains, then a fixed LDS tree (the
// shape of pod.hip's pod_mean_kernel). One block.
__global__ __launch_bounds__(NT)
void cos_sum_kernel(const float* __restrict__ v, float* __restrict__ out, int n,
                    float scale) {
  __shared__ float red[NT];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += NT) s += v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * scale;
}

static bool cos_shape_ok(int rows, int D, int is_fp32) {
  return rows >= 1 && D >= 1 && D <= COS_MAX_D &&
         D % (is_fp32 ? 4 : 8) == 0;
}

extern "C" {

// 1 when the launchers below accept the shape: rows >= 1, 1 <= D <= 2048,
// D % 8 == 0 for bf16 rows, D % 4 == 0 for fp32 rows
int cilfw_cosine_supported(int rows, int D, int is_fp32) {
  return cos_shape_ok(rows, D, is_fp32) ? 1 : 0;
}

// x (rows, D) bf16 or fp32 -> y bf16 (rows, D) = scale[0] * x r(x), rinv fp32
// (rows). scale: 1 fp32 on the device, or null for 1. Every element of y and
// rinv is written. Returns 0, or 1 when the shape is refused (no launch).
int cilfw_rownorm_fwd(const void* x, const void* scale, void* y, void* rinv,
                      int rows, int D, int is_fp32, void* stream) {
  if (!cos_shape_ok(rows, D, is_fp32)) return 1;
  const dim3 grid(cdiv(rows, COS_ROWS));
  hipStream_t st = (hipStream_t)stream;
  if (is_fp32)
    hipLaunchKernelGGL(rownorm_fwd_kernel<true>, grid, dim3(NT), 0, st,
                       (const float*)x, (const float*)scale, (bf16_t*)y,
                       (float*)rinv, rows, D);
  else
    hipLaunchKernelGGL(rownorm_fwd_kernel<false>, grid, dim3(NT), 0, st,
                       (const bf16_t*)x, (const float*)scale, (bf16_t*)y,
                       (float*)rinv, rows, D);
  return 0;
}

// dx = (scale[0] rinv) (G - x^ (x^ . G)), x^ = x rinv, in the type of x (G
// has that type too); dsig fp32 (rows) = x^ . G, or null. scale as above.
int cilfw_rownorm_bwd(const void* x, const void* rinv, const void* G,
                      const void* scale, void* dx, void* dsig, int rows, int D,
                      int is_fp32, void* stream) {
  if (!cos_shape_ok(rows, D, is_fp32)) return 1;
  const dim3 grid(cdiv(rows, COS_ROWS));
  hipStream_t st = (hipStream_t)stream;
  if (is_fp32)
    hipLaunchKernelGGL(rownorm_bwd_kernel<true>, grid, dim3(NT), 0, st,
                       (const float*)x, (const float*)rinv, (const float*)G,
                       (const float*)scale, (float*)dx, (float*)dsig, rows, D);
  else
    hipLaunchKernelGGL(rownorm_bwd_kernel<false>, grid, dim3(NT), 0, st,
                       (const bf16_t*)x, (const float*)rinv, (const bf16_t*)G,
                       (const float*)scale, (bf16_t*)dx, (float*)dsig, rows,
                       D);
  return 0;
}

// out[0] = scale * sum of v[0..n)
int cilfw_cos_sum(const void* v, void* out, int n, float scale, void* stream) {
  if (n < 1) return 1;
  hipLaunchKernelGGL(cos_sum_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream,
                     (const float*)v, (float*)out, n, scale);
  return 0;
}

// s, t bf16 (M, D) -> gs fp32 (M, D) for upstream 1, l fp32 (M), loss fp32
// (1) = mean_m l.
int cilfw_flat_dist(const void* s, const void* t, void* gs, void* l,
                    void* loss, int M, int D, void* stream) {
  if (!cos_shape_ok(M, D, 0)) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flat_dist_kernel, dim3(cdiv(M, COS_ROWS)), dim3(NT), 0,
                     st, (const bf16_t*)s, (const bf16_t*)t, (float*)gs,
                     (float*)l, M, D, 1.f / (float)M);
  hipLaunchKernelGGL(cos_sum_kernel, dim3(1), dim3(NT), 0, st,
                     (const float*)l, (float*)loss, M, 1.f / (float)M);
  return 0;
}

// ds bf16 (M, D) = up[0] * gs; up: 1 fp32 on the device.
int cilfw_flat_bwd(const void* gs, const void* up, void* ds, int M, int D,
                   void* stream) {
  if (!cos_shape_ok(M, D, 0)) return 1;
  const long items = (long)M * (D / 8);
  const long blocks = (items + NT - 1) / NT;
  if (blocks > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(flat_bwd_kernel, dim3((unsigned)blocks), dim3(NT), 0,
                     (hipStream_t)stream, (const float*)gs, (const float*)up,
                     (bf16_t*)ds, items);
  return 0;
}

}  // extern "C"
