// cilfw — device-side data path: fused gather -> affine bilinear resample ->
// horizontal flip -> quantize -> normalize, one launch per batch.
//
// Output pixel (i, j) of sample n reads the uint8 source image idx[n] at
//   fy = oy + i*sy,  fx = ox + jj*sx   (jj = S-1-j when flip[n], else j)
// with (oy, ox, sy, sx) = params[n]. RandomResizedCrop, the eval
// resize+center-crop and a plain resize are all this one affine form, so the
// kernel has no per-transform cases (cilfw/data/device_augment.py builds the
// parameter rows).
//
// Thread mapping. The output [N, S, S, C] is treated as one flat array and
// every lane owns 16 consecutive BYTES of it (16 uint8 / 8 bf16 / 4 fp32
// elements), stored with a single aligned 16-byte vector store: a wave writes
// 1 KiB contiguous per store instruction whatever S and C are. ([S, S, 3] rows
// are 16-byte aligned neither per pixel nor per row, so a per-pixel or per-row
// mapping would need peeled scalar heads and tails.) A lane decodes
// (n, i, j, c) of its first element once and then walks: the sample state
// (params, flip, source base), the row state (y0, y1, ty) and the pixel state
// (x0, x1, tx) are each recomputed only when the walk crosses into a new
// sample / row / pixel, which for 16 bytes is almost never more than one row.
// Source reads are 4 byte loads per element from an image that stays in L2
// (a 256x256x3 source is 192 KiB); the kernel is bound by the output stream.
//
// Arithmetic is fp32 with contraction OFF so it rounds exactly like the
// torch reference in cilfw/ops/functional.py (a + t*(b - a), x first, then
// y; clamp to [0, 255]; floor).
#include "common.h"

#define DNT 256

enum { OUT_U8 = 0, OUT_F32 = 1, OUT_BF16 = 2 };

template <int MODE> struct OutVec;
template <> struct OutVec<OUT_U8> { typedef uint8_t T; enum { V = 16 }; };
template <> struct OutVec<OUT_F32> { typedef float T; enum { V = 4 }; };
template <> struct OutVec<OUT_BF16> { typedef bf16_t T; enum { V = 8 }; };

template <int MODE>
DEV typename OutVec<MODE>::T out_cvt(float level, const float* mean255,
                                     const float* std255, int c) {
#pragma clang fp contract(off)
  if (MODE == OUT_U8) return (typename OutVec<MODE>::T)level;
  float v = (level - mean255[c]) / std255[c];
  if (MODE == OUT_F32) return (typename OutVec<MODE>::T)v;
  return (typename OutVec<MODE>::T)f2bf(v);
}

// Source accessors. The kernel body is shared; what differs is where sample m
// lives and how large it is. Dense: one [M,Hs,Ws,C] tensor, geometry uniform
// (kernel constants after inlining). Ragged: a flat byte pool with per-image
// byte offsets and (H, W); image m is H*W*C contiguous HWC bytes at
// pool + offsets[m].
struct DenseSrc {
  const uint8_t* src;
  int Hs, Ws;
  long img_elems;
  DEV void sample(long m, const uint8_t*& base, int& H, int& W) const {
    base = src + m * img_elems;
    H = Hs;
    W = Ws;
  }
};

struct RaggedSrc {
  const uint8_t* pool;
  const int64_t* offsets;
  const int* hw;
  DEV void sample(long m, const uint8_t*& base, int& H, int& W) const {
    base = pool + offsets[m];
    H = hw[2 * m];
    W = hw[2 * m + 1];
  }
};

// A lane's 16 bytes may straddle two samples. With a ragged source those two
// samples differ in H, W and base, so EVERYTHING derived from the image is
// per-sample state reloaded at the new_sample transition: the clamp limits
// (ymax, xmax, Hs, Ws) and the row stride here, and - because a new sample
// always starts a new row and a new pixel - the row pointers and x offsets
// right below it in the same iteration.
template <int MODE, class Src>
DEV void crop_resize_body(const Src& source,
                          const int64_t* __restrict__ idx,
                          const float* __restrict__ params,
                          const uint8_t* __restrict__ flip,
                          const float* __restrict__ mean255,
                          const float* __restrict__ std255,
                          typename OutVec<MODE>::T* __restrict__ out,
                          int M, int C, int S, long total) {
#pragma clang fp contract(off)
  typedef typename OutVec<MODE>::T T;
  constexpr int V = OutVec<MODE>::V;
  long e0 = ((long)blockIdx.x * DNT + threadIdx.x) * V;
  if (e0 >= total) return;
  int nv = (total - e0 < V) ? (int)(total - e0) : V;

  const int rowlen = S * C;
  const long per = (long)S * rowlen;
  int n = (int)(e0 / per);
  int rem = (int)(e0 - (long)n * per);
  int i = rem / rowlen;
  int q = rem - i * rowlen;
  int j = q / C;
  int c = q - j * C;

  float oy = 0.f, ox = 0.f, sy = 0.f, sx = 0.f, ty = 0.f, tx = 0.f;
  bool fl = false;
  // per-sample source state
  const uint8_t* base = nullptr;
  int Hs = 1, Ws = 1, row_elems = 0;
  float ymax = 0.f, xmax = 0.f;
  const uint8_t *r0 = nullptr, *r1 = nullptr;  // rows y0 / y1 of the sample
  int xo0 = 0, xo1 = 0;                // element offsets of x0 / x1 in a row
  bool new_sample = true, new_row = true, new_pix = true;

  __attribute__((aligned(16))) T vals[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (k < nv) {
      if (new_sample) {
        const float* p = params + (long)n * 4;
        oy = p[0]; ox = p[1]; sy = p[2]; sx = p[3];
        fl = flip[n] != 0;
        long m = idx ? (long)idx[n] : (long)n;
        m = m < 0 ? 0 : (m > M - 1 ? M - 1 : m);  // never read outside src
        source.sample(m, base, Hs, Ws);
        row_elems = Ws * C;
        ymax = (float)(Hs - 1);
        xmax = (float)(Ws - 1);
        new_sample = false;
      }
      if (new_row) {
        float fy = oy + (float)i * sy;
        float y0f = fmaxf(fminf(floorf(fy), ymax), 0.f);
        int y0 = (int)y0f;
        int y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1;
        ty = fy - y0f;
        r0 = base + (long)y0 * row_elems;
        r1 = base + (long)y1 * row_elems;
        new_row = false;
      }
      if (new_pix) {
        int jj = fl ? S - 1 - j : j;
        float fx = ox + (float)jj * sx;
        float x0f = fmaxf(fminf(floorf(fx), xmax), 0.f);
        int x0 = (int)x0f;
        int x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1;
        tx = fx - x0f;
        xo0 = x0 * C;
        xo1 = x1 * C;
        new_pix = false;
      }
      float a = (float)r0[xo0 + c], b = (float)r0[xo1 + c];
      float d = (float)r1[xo0 + c], e = (float)r1[xo1 + c];
      float top = a + tx * (b - a);
      float bot = d + tx * (e - d);
      float v = top + ty * (bot - top);
      v = floorf(fminf(fmaxf(v, 0.f), 255.f));
      vals[k] = out_cvt<MODE>(v, mean255, std255, c);
      if (++c == C) {
        c = 0;
        new_pix = true;
        if (++j == S) {
          j = 0;
          new_row = true;
          if (++i == S) {
            i = 0;
            ++n;
            new_sample = true;
          }
        }
      }
    }
  }

  if (nv == V) {
    *(int4*)&out[e0] = *(const int4*)vals;  // e0*sizeof(T) is a multiple of 16
  } else {
    for (int k = 0; k < nv; ++k) out[e0 + k] = vals[k];
  }
}

template <int MODE>
__global__ __launch_bounds__(DNT)
void crop_resize_kernel(const uint8_t* __restrict__ src,
                        const int64_t* __restrict__ idx,
                        const float* __restrict__ params,
                        const uint8_t* __restrict__ flip,
                        const float* __restrict__ mean255,
                        const float* __restrict__ std255,
                        typename OutVec<MODE>::T* __restrict__ out,
                        int M, int N, int Hs, int Ws, int C, int S,
                        long total) {
  DenseSrc source = {src, Hs, Ws, (long)Hs * Ws * C};
  crop_resize_body<MODE>(source, idx, params, flip, mean255, std255, out, M,
                         C, S, total);
}

template <int MODE>
__global__ __launch_bounds__(DNT)
void crop_resize_ragged_kernel(const uint8_t* __restrict__ pool,
                               const int64_t* __restrict__ offsets,
                               const int* __restrict__ hw,
                               const int64_t* __restrict__ idx,
                               const float* __restrict__ params,
                               const uint8_t* __restrict__ flip,
                               const float* __restrict__ mean255,
                               const float* __restrict__ std255,
                               typename OutVec<MODE>::T* __restrict__ out,
                               int M, int C, int S, long total) {
  RaggedSrc source = {pool, offsets, hw};
  crop_resize_body<MODE>(source, idx, params, flip, mean255, std255, out, M,
                         C, S, total);
}

extern "C" {

// src uint8 [M,Hs,Ws,C]; idx int64 [N] or null (identity, N == M);
// params fp32 [N,4]; flip uint8 [N]; mean255/std255 fp32 [C] (unused in uint8
// mode); out [N,S,S,C], 16-byte aligned. out_mode: 0 uint8 levels, 1 fp32
// normalized, 2 bf16 normalized.
void cilfw_crop_resize(const void* src, const void* idx, const void* params,
                       const void* flip, const void* mean255,
                       const void* std255, void* out, int M, int N, int Hs,
                       int Ws, int C, int S, int out_mode, void* stream) {
  long total = (long)N * S * S * C;
  if (total <= 0) return;
#define CILFW_CR_LAUNCH(MODE)                                                 \
  hipLaunchKernelGGL(                                                         \
      crop_resize_kernel<MODE>,                                               \
      dim3((unsigned)((total + (long)DNT * OutVec<MODE>::V - 1) /             \
                      ((long)DNT * OutVec<MODE>::V))),                        \
      dim3(DNT), 0, (hipStream_t)stream, (const uint8_t*)src,                 \
      (const int64_t*)idx, (const float*)params, (const uint8_t*)flip,        \
      (const float*)mean255, (const float*)std255,                            \
      (OutVec<MODE>::T*)out, M, N, Hs, Ws, C, S, total)
  if (out_mode == OUT_U8) CILFW_CR_LAUNCH(OUT_U8);
  else if (out_mode == OUT_F32) CILFW_CR_LAUNCH(OUT_F32);
  else CILFW_CR_LAUNCH(OUT_BF16);
#undef CILFW_CR_LAUNCH
}

// The same over a ragged source: pool uint8 flat bytes; offsets int64 [M]
// (byte offset of image m, honoured as given); hw int32 [M,2] = (H, W); image
// m is H*W*C contiguous HWC bytes. idx int64 [N] (required); the rest as
// cilfw_crop_resize. The caller guarantees offsets[m] + H*W*C <= pool size
// and H*W*C < 2^31 for every m (checked once where the pool is built).
void cilfw_crop_resize_ragged(const void* pool, const void* offsets,
                              const void* hw, const void* idx,
                              const void* params, const void* flip,
                              const void* mean255, const void* std255,
                              void* out, int M, int N, int C, int S,
                              int out_mode, void* stream) {
  long total = (long)N * S * S * C;
  if (total <= 0 || M <= 0) return;
#define CILFW_CRR_LAUNCH(MODE)                                                \
  hipLaunchKernelGGL(                                                         \
      crop_resize_ragged_kernel<MODE>,                                        \
      dim3((unsigned)((total + (long)DNT * OutVec<MODE>::V - 1) /             \
                      ((long)DNT * OutVec<MODE>::V))),                        \
      dim3(DNT), 0, (hipStream_t)stream, (const uint8_t*)pool,                \
      (const int64_t*)offsets, (const int*)hw, (const int64_t*)idx,           \
      (const float*)params, (const uint8_t*)flip, (const float*)mean255,      \
      (const float*)std255, (OutVec<MODE>::T*)out, M, C, S, total)
  if (out_mode == OUT_U8) CILFW_CRR_LAUNCH(OUT_U8);
  else if (out_mode == OUT_F32) CILFW_CRR_LAUNCH(OUT_F32);
  else CILFW_CRR_LAUNCH(OUT_BF16);
#undef CILFW_CRR_LAUNCH
}

}  // extern "C"
