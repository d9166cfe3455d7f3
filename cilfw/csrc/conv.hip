// cilfw — implicit-GEMM MFMA convolutions for gfx950 (CDNA4), NHWC bf16.
//
// Replaces the reference's cuDNN conv kernels.
// Formulation: Y[M=N*Ho*Wo, K] = im2col(X)[M, C*R*S] @ W[C*R*S, K], W stored
// (R,S,C,K) so the B operand is dense with k-index (r*S+s)*C+c.
//
// Tile: 128(M) x 64(Kout) x BKT(K-step), 4 waves as 2x2, each wave 64x32 via
// mfma_f32_16x16x32_bf16 (M_rep=4, N_rep=2), fp32 accumulators, double-buffered
// LDS with +16B row padding (bank-conflict-free ds_read_b128). BKT is a
// template parameter: 64 when the K loop is long enough (halves the barrier
// count, 16 MFMAs between barriers), 32 for short-K convs (stems, 1x1).
//
// Late layers have small M (batch x 4x4 spatial) and huge K-dim (C*R*S up to
// 4608): too few workgroups to fill 256 CUs. When (M-blocks x K-blocks) is
// small the launcher SPLITS the K loop over blockIdx.z; each slice writes an
// fp32 partial slab and a reduce kernel sums slabs -> bf16 (no atomics).
// Backward-weight always uses the slab path (it is a huge-reduction GEMM).

#include "common.h"

#define BM 128
#define BN 64
#define NTHREADS 256

struct ConvGeom {
  int N, H, W, C, K, R, S, stride, pad, pad2, Ho, Wo;  // pad2 = w-axis pad
  // round-up magic multipliers for division by Ho*Wo and Wo in per-K-step
  // gathers (exact for n < 2^22, divisor < 2^14 — launcher asserts):
  // q = (n * m) >> 40 == n / d. Runtime-divisor division otherwise expands
  // to a ~40-instruction v_rcp sequence inside the hot loop.
  unsigned long long m_howo, m_wo;
  // slow-path (tiny-C / ragged) per-element decode divisors: k/(C or K), rs/S
  unsigned long long m_ck, m_s;
};

static inline unsigned long long magic40(int d) {
  return d > 0 ? ((1ULL << 40) / (unsigned)d + 1) : 0;
}

DEV unsigned mdiv40(unsigned n, unsigned long long m) {
  return (unsigned)(((unsigned long long)n * m) >> 40);
}

// sum ksplit fp32 slabs [ns][len] -> bf16 out[len]
__global__ __launch_bounds__(NTHREADS)
void reduce_slabs_bf16_kernel(const float* __restrict__ ws,
                              bf16_t* __restrict__ out, int ns, long len) {
  long i0 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 4;
  if (i0 >= len) return;
  if (i0 + 4 <= len) {
    float4 acc = *(const float4*)&ws[i0];
    for (int s = 1; s < ns; ++s) {
      float4 v = *(const float4*)&ws[(long)s * len + i0];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    bf16_t o[4] = {f2bf(acc.x), f2bf(acc.y), f2bf(acc.z), f2bf(acc.w)};
    *(int2*)&out[i0] = *(int2*)o;
  } else {
    for (long i = i0; i < len; ++i) {
      float a = ws[i];
      for (int s = 1; s < ns; ++s) a += ws[(long)s * len + i];
      out[i] = f2bf(a);
    }
  }
}

// sum ksplit fp32 slabs -> fp32 out (weight grads); accum adds into out
// (grad-accumulation steps deliver straight into the flat grad slot)
__global__ __launch_bounds__(NTHREADS)
void reduce_slabs_f32_kernel(const float* __restrict__ ws,
                             float* __restrict__ out, int ns, long len,
                             int accum) {
  long i0 = ((long)blockIdx.x * NTHREADS + threadIdx.x) * 4;
  if (i0 >= len) return;
  if (i0 + 4 <= len) {
    float4 acc = *(const float4*)&ws[i0];
    for (int s = 1; s < ns; ++s) {
      float4 v = *(const float4*)&ws[(long)s * len + i0];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (accum) {
      float4 o = *(const float4*)&out[i0];
      acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
    }
    *(float4*)&out[i0] = acc;
  } else {
    for (long i = i0; i < len; ++i) {
      float a = ws[i];
      for (int s = 1; s < ns; ++s) a += ws[(long)s * len + i];
      out[i] = accum ? out[i] + a : a;
    }
  }
}

// ============================== forward ==============================

// Branchless OOB handling: gather loads use a CLAMPED (always-valid) address
// and the loaded value is zeroed by cndmask when out of bounds. The
// conditional-load form compiles to exec-mask branches around every load
// (63 s_and_saveexec waterfalls in the round-1 K-loop, 1758-instruction body
// for 8 MFMAs); the select form keeps the loop straight-line.
__device__ __forceinline__ int4 masked_i4(int4 v, bool ok) {
  int4 z{0, 0, 0, 0};
  return ok ? v : z;
}

template <int BKT, int BMX = BM, int BNX = BN, bool FAST = true>
__global__ __launch_bounds__(NTHREADS)
void conv2d_fwd_kernel(const bf16_t* __restrict__ x,
                       const bf16_t* __restrict__ w,
                       bf16_t* __restrict__ y, float* __restrict__ ws,
                       ConvGeom g, int M, int CRS, int nk, int ksplit) {
  constexpr int NQ = BKT / 32;      // 16-elem chunks per thread in A staging
  constexpr int LPX = BKT + 8;
  constexpr int NR = BMX / 128;     // A-tile rows per thread (1 or 2)
  constexpr int MR = BMX / 32;      // M-fragments per wave (4 or 8)
  constexpr int NRC = BNX / 32;     // N-fragments per wave (2 or 4)
  __shared__ bf16_t lds[2 * BMX * LPX + 2 * BNX * LPX];
  const int AS0 = 0, BS0 = 2 * BMX * LPX;
  const int m0 = blockIdx.x * BMX;
  const int ko0 = blockIdx.y * BNX;
  const int t = threadIdx.x;
  const int wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int steps = (nk + ksplit - 1) / ksplit;
  const int kt0 = blockIdx.z * steps;
  const int kt1 = min(kt0 + steps, nk);

  const int arow = t >> 1, ahalf = t & 1;
  int an[NR], ahb[NR], awb[NR];
  bool arow_ok[NR];
#pragma unroll
  for (int rr = 0; rr < NR; ++rr) {
    int m = m0 + arow + rr * 128;
    arow_ok[rr] = m < M;
    int mc = min(m, M - 1);  // clamped: address math always valid
    int n = mc / (g.Ho * g.Wo);
    int rem = mc - n * (g.Ho * g.Wo);
    int aho = rem / g.Wo;
    int awo = rem - aho * g.Wo;
    an[rr] = n;
    ahb[rr] = aho * g.stride - g.pad;
    awb[rr] = awo * g.stride - g.pad2;
  }

  f32x4 acc[MR][NRC];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NRC; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  int4 areg[NR][2 * NQ];
  __align__(16) bf16_t breg[NQ][BNX / 64][8];

  // incremental im2col decomposition (fast path): per q-chunk (r, s, c0)
  // advance by compare/sub each K-step instead of div/mod every call
  int inc_r[NQ], inc_s[NQ], inc_c0[NQ];
  if (FAST) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int k = kt0 * BKT + q * 32 + ahalf * 16;
      int rs = k / g.C;
      inc_c0[q] = k - rs * g.C;
      inc_r[q] = rs / g.S;
      inc_s[q] = rs - inc_r[q] * g.S;
    }
  }

  auto stage_to_regs = [&](int kt) {
    const int k0 = kt * BKT;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      // A chunk: 16 elems at col q*32 + ahalf*16 (within one (r,s): C%16==0)
      if (FAST) {
        int c0 = inc_c0[q], r = inc_r[q], s = inc_s[q];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
          int hi = ahb[rr] + r, wi = awb[rr] + s;
          bool ok = arow_ok[rr] & ((unsigned)hi < (unsigned)g.H)
                    & ((unsigned)wi < (unsigned)g.W);
          int hic = min(max(hi, 0), g.H - 1);
          int wic = min(max(wi, 0), g.W - 1);
          const int4* src = (const int4*)&x[(((long)an[rr] * g.H + hic)
                                             * g.W + wic) * g.C + c0];
          areg[rr][2 * q] = masked_i4(src[0], ok);
          areg[rr][2 * q + 1] = masked_i4(src[1], ok);
        }
        c0 += BKT;
        while (c0 >= g.C) {
          c0 -= g.C;
          if (++s == g.S) { s = 0; ++r; }
        }
        inc_c0[q] = c0; inc_r[q] = r; inc_s[q] = s;
      } else {
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
          __align__(16) bf16_t tmp[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            int k = k0 + q * 32 + ahalf * 16 + j;
            int kc = min(k, CRS - 1);
            int rs = (int)mdiv40((unsigned)kc, g.m_ck);
            int c = kc - rs * g.C;
            int r = (int)mdiv40((unsigned)rs, g.m_s);
            int s = rs - r * g.S;
            int hi = ahb[rr] + r, wi = awb[rr] + s;
            bool ok = arow_ok[rr] & (k < CRS)
                      & ((unsigned)hi < (unsigned)g.H)
                      & ((unsigned)wi < (unsigned)g.W);
            int hic = min(max(hi, 0), g.H - 1);
            int wic = min(max(wi, 0), g.W - 1);
            bf16_t v = x[(((long)an[rr] * g.H + hic) * g.W + wic) * g.C + c];
            tmp[j] = ok ? v : (bf16_t)0;
          }
          areg[rr][2 * q] = *(int4*)&tmp[0];
          areg[rr][2 * q + 1] = *(int4*)&tmp[8];
        }
      }
      // B chunk: thread owns one Bs row (cout n) per 64-col group and 8 k's:
      // strided reads coalesce ACROSS lanes (n contiguous); each LDS write is
      // one b128 (conflict-free 8-lane groups).
#pragma unroll
      for (int h = 0; h < BNX / 64; ++h) {
        const int bn = (t & 63) + h * 64;
        const int bk8 = ((t >> 6) & 3) * 8 + q * 32;
        const bool n_ok = ko0 + bn < g.K;
        const int bcol = min(ko0 + bn, g.K - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int k = k0 + bk8 + j;
          bool ok = n_ok & (k < CRS);
          bf16_t v = w[(long)min(k, CRS - 1) * g.K + bcol];
          breg[q][h][j] = ok ? v : (bf16_t)0;
        }
      }
    }
  };

  auto regs_to_lds = [&](int buf) {
    bf16_t* As = &lds[AS0 + buf * BMX * LPX];
    bf16_t* Bs = &lds[BS0 + buf * BN * LPX];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) {
        *(int4*)&As[(arow + rr * 128) * LPX + q * 32 + ahalf * 16] =
            areg[rr][2 * q];
        *(int4*)&As[(arow + rr * 128) * LPX + q * 32 + ahalf * 16 + 8] =
            areg[rr][2 * q + 1];
      }
#pragma unroll
      for (int h = 0; h < BNX / 64; ++h) {
        const int bn = (t & 63) + h * 64;
        const int bk8 = ((t >> 6) & 3) * 8 + q * 32;
        *(int4*)&Bs[bn * LPX + bk8] = *(int4*)breg[q][h];
      }
    }
  };

  if (kt0 < kt1) {
    stage_to_regs(kt0);
    regs_to_lds(0);
  }
  __syncthreads();
  FragIdx fi = frag_idx();
  for (int kt = kt0; kt < kt1; ++kt) {
    int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) stage_to_regs(kt + 1);
    {
      const bf16_t* As = &lds[AS0 + cur * BMX * LPX];
      const bf16_t* Bs = &lds[BS0 + cur * BN * LPX];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int kb = fi.quad * 8 + q * 32;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
          int row = wr * (BMX / 2) + mr * 16 + fi.half;
          bf16x8 a = *(const bf16x8*)&As[row * LPX + kb];
#pragma unroll
          for (int nr = 0; nr < NRC; ++nr) {
            int col = wc * (BNX / 2) + nr * 16 + fi.half;
            bf16x8 b = *(const bf16x8*)&Bs[col * LPX + kb];
            acc[mr][nr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b, acc[mr][nr], 0, 0, 0);
          }
        }
      }
    }
    // single barrier per K-step: writes target buf[cur^1], whose readers all
    // finished before the PREVIOUS barrier — the post-MFMA barrier is
    // unnecessary (fast waves cannot overwrite buf[cur]: the next write to it
    // happens after this barrier, which slow readers must reach first)
    if (kt + 1 < kt1) {
      regs_to_lds(cur ^ 1);
      __syncthreads();
    }
  }

#pragma unroll
  for (int mr = 0; mr < MR; ++mr)
#pragma unroll
    for (int nr = 0; nr < NRC; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * (BMX / 2) + mr * 16 + fi.quad * 4 + r;
        int col = ko0 + wc * (BNX / 2) + nr * 16 + fi.half;
        if (row < M && col < g.K) {
          if (ksplit > 1)
            ws[((long)blockIdx.z * M + row) * g.K + col] = acc[mr][nr][r];
          else
            y[(long)row * g.K + col] = f2bf(acc[mr][nr][r]);
        }
      }
}

// ============================== backward data ==============================
// dX[M=N*H*W, C] = gather(dY)[M, R*S*K] @ B where B[(r,s,k)][c] = W[r,s,c,k].

template <int BKT, bool FAST = true, bool BNP = false>
__global__ __launch_bounds__(NTHREADS)
void conv2d_bwd_data_kernel(const bf16_t* __restrict__ dy,
                            const bf16_t* __restrict__ w,
                            bf16_t* __restrict__ dx, float* __restrict__ ws,
                            ConvGeom g, int M, int RSK, int nk, int ksplit,
                            // BNP epilogue: per-block (dgamma, dbeta)
                            // partials of the downstream training BN whose
                            // backward consumes this dx as its dy (the BN's
                            // own sums pass is then skipped — mirror of the
                            // fwd-side conv->bn_parts fusion)
                            const bf16_t* __restrict__ bn_y = nullptr,
                            const bf16_t* __restrict__ bn_x = nullptr,
                            const float* __restrict__ bn_mean = nullptr,
                            const float* __restrict__ bn_invstd = nullptr,
                            float* __restrict__ bn_parts = nullptr,
                            int bn_relu = 0) {
  constexpr int NQ = BKT / 32;
  constexpr int LPX = BKT + 8;
  __shared__ bf16_t lds[2 * BM * LPX + 2 * BN * LPX];
  const int AS0 = 0, BS0 = 2 * BM * LPX;
  const int m0 = blockIdx.x * BM;
  const int c0 = blockIdx.y * BN;
  const int t = threadIdx.x;
  const int wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int steps = (nk + ksplit - 1) / ksplit;
  const int kt0 = blockIdx.z * steps;
  const int kt1 = min(kt0 + steps, nk);

  const int arow = t >> 1, ahalf = t & 1;
  int m = m0 + arow;
  bool arow_ok = m < M;
  int mc = min(m, M - 1);
  int an = mc / (g.H * g.W);
  int mrem = mc - an * (g.H * g.W);
  int ahi = mrem / g.W;
  int awi = mrem - ahi * g.W;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  int4 areg[2 * NQ];
  __align__(16) bf16_t breg[NQ][8];

  int inc_r[NQ], inc_s[NQ], inc_kc[NQ];
  // B-gather incremental state (c row fixed = t>>2; k advances by BKT/step)
  int binc_rs[NQ], binc_kc[NQ];
  if (FAST) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int k = kt0 * BKT + q * 32 + ahalf * 16;
      int rs = k / g.K;
      inc_kc[q] = k - rs * g.K;
      inc_r[q] = rs / g.S;
      inc_s[q] = rs - inc_r[q] * g.S;
      int bk = kt0 * BKT + (t & 3) * 8 + q * 32;
      binc_rs[q] = bk / g.K;
      binc_kc[q] = bk - binc_rs[q] * g.K;
    }
  }

  auto stage_to_regs = [&](int kt) {
    const int k0 = kt * BKT;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (FAST) {  // K % 16 == 0: a 16-chunk stays inside one (r,s)
        int kc0 = inc_kc[q], r = inc_r[q], s = inc_s[q];
        int ho2 = ahi + g.pad - r, wo2 = awi + g.pad2 - s;
        // stride is 1 or 2 everywhere cilfw launches this: a shift-select
        // replaces the runtime division (a ~40-instruction expansion here)
        const bool s2d = g.stride == 2;
        int ho = s2d ? (ho2 >> 1) : ho2;
        int wo = s2d ? (wo2 >> 1) : wo2;
        bool par = !s2d | (((ho2 | wo2) & 1) == 0);
        bool ok = arow_ok & (ho2 >= 0) & (wo2 >= 0) & par &
                  (ho < g.Ho) & (wo < g.Wo);
        int hoc = min(max(ho, 0), g.Ho - 1);
        int woc = min(max(wo, 0), g.Wo - 1);
        const int4* src = (const int4*)&dy[(((long)an * g.Ho + hoc) * g.Wo
                                            + woc) * g.K + kc0];
        areg[2 * q] = masked_i4(src[0], ok);
        areg[2 * q + 1] = masked_i4(src[1], ok);
        kc0 += BKT;
        while (kc0 >= g.K) {
          kc0 -= g.K;
          if (++s == g.S) { s = 0; ++r; }
        }
        inc_kc[q] = kc0; inc_r[q] = r; inc_s[q] = s;
      } else {
        __align__(16) bf16_t tmp[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          int k = k0 + q * 32 + ahalf * 16 + j;
          int kk = min(k, RSK - 1);
          int rs = (int)mdiv40((unsigned)kk, g.m_ck);
          int kc = kk - rs * g.K;
          int r = (int)mdiv40((unsigned)rs, g.m_s);
          int s = rs - r * g.S;
          int ho2 = ahi + g.pad - r, wo2 = awi + g.pad2 - s;
          const bool s2d = g.stride == 2;
          int ho = s2d ? (ho2 >> 1) : ho2;
          int wo = s2d ? (wo2 >> 1) : wo2;
          bool par = !s2d | (((ho2 | wo2) & 1) == 0);
          bool ok = arow_ok & (k < RSK) & (ho2 >= 0) & (wo2 >= 0) & par
                    & (ho < g.Ho) & (wo < g.Wo);
          int hoc = min(max(ho, 0), g.Ho - 1);
          int woc = min(max(wo, 0), g.Wo - 1);
          bf16_t v = dy[(((long)an * g.Ho + hoc) * g.Wo + woc) * g.K + kc];
          tmp[j] = ok ? v : (bf16_t)0;
        }
        areg[2 * q] = *(int4*)&tmp[0];
        areg[2 * q + 1] = *(int4*)&tmp[8];
      }
      // B: thread c = t>>2 (0..63), slot = t&3 -> 8 contiguous kc (K % 8 == 0)
      const int bc = t >> 2, bkk = (t & 3) * 8 + q * 32;
      int k = k0 + bkk;
      const int bcc = min(c0 + bc, g.C - 1);
      if (FAST) {
        int rs = binc_rs[q], kc = binc_kc[q];
        bool ok = (k < RSK) & (c0 + bc < g.C);
        int rsc = min(rs, g.R * g.S - 1);
        const int4* src = (const int4*)&w[((long)rsc * g.C + bcc) * g.K + kc];
        *(int4*)breg[q] = masked_i4(*src, ok);
        kc += BKT;
        while (kc >= g.K) { kc -= g.K; ++rs; }
        binc_rs[q] = rs; binc_kc[q] = kc;
      } else if (k < RSK && c0 + bc < g.C) {
        int rs = k / g.K, kc = k - rs * g.K;
        *(int4*)breg[q] = *(const int4*)&w[((long)rs * g.C + c0 + bc) * g.K
                                           + kc];
      } else {
        *(int4*)breg[q] = int4{0, 0, 0, 0};
      }
    }
  };

  auto regs_to_lds = [&](int buf) {
    bf16_t* As = &lds[AS0 + buf * BM * LPX];
    bf16_t* Bs = &lds[BS0 + buf * BN * LPX];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      *(int4*)&As[arow * LPX + q * 32 + ahalf * 16] = areg[2 * q];
      *(int4*)&As[arow * LPX + q * 32 + ahalf * 16 + 8] = areg[2 * q + 1];
      const int bc = t >> 2, bkk = (t & 3) * 8 + q * 32;
      *(int4*)&Bs[bc * LPX + bkk] = *(int4*)breg[q];
    }
  };

  if (kt0 < kt1) {
    stage_to_regs(kt0);
    regs_to_lds(0);
  }
  __syncthreads();
  FragIdx fi = frag_idx();
  for (int kt = kt0; kt < kt1; ++kt) {
    int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) stage_to_regs(kt + 1);
    {
      const bf16_t* As = &lds[AS0 + cur * BM * LPX];
      const bf16_t* Bs = &lds[BS0 + cur * BN * LPX];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int kb = fi.quad * 8 + q * 32;
#pragma unroll
        for (int mr = 0; mr < 4; ++mr) {
          int row = wr * 64 + mr * 16 + fi.half;
          bf16x8 a = *(const bf16x8*)&As[row * LPX + kb];
#pragma unroll
          for (int nr = 0; nr < 2; ++nr) {
            int col = wc * 32 + nr * 16 + fi.half;
            bf16x8 b = *(const bf16x8*)&Bs[col * LPX + kb];
            acc[mr][nr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b, acc[mr][nr], 0, 0, 0);
          }
        }
      }
    }
    // single barrier per K-step: writes target buf[cur^1], whose readers all
    // finished before the PREVIOUS barrier — the post-MFMA barrier is
    // unnecessary (fast waves cannot overwrite buf[cur]: the next write to it
    // happens after this barrier, which slow readers must reach first)
    if (kt + 1 < kt1) {
      regs_to_lds(cur ^ 1);
      __syncthreads();
    }
  }

  float bnmu[2], bnis[2], bnsg[2] = {0.f, 0.f}, bnsb[2] = {0.f, 0.f};
  if (BNP) {
#pragma unroll
    for (int nr = 0; nr < 2; ++nr) {
      int cc = min(c0 + wc * 32 + nr * 16 + fi.half, g.C - 1);
      bnmu[nr] = bn_mean[cc];
      bnis[nr] = bn_invstd[cc];
    }
  }
#pragma unroll
  for (int mr = 0; mr < 4; ++mr)
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mr * 16 + fi.quad * 4 + r;
        int col = c0 + wc * 32 + nr * 16 + fi.half;
        if (row < M && col < g.C) {
          if (!BNP && ksplit > 1) {
            ws[((long)blockIdx.z * M + row) * g.C + col] = acc[mr][nr][r];
          } else {
            bf16_t h = f2bf(acc[mr][nr][r]);
            dx[(long)row * g.C + col] = h;
            if (BNP) {
              long i = (long)row * g.C + col;
              // mask with the BN's post-ReLU output (this conv's input)
              // and round through bf16 first: identical math to the
              // standalone bn_bwd_sums pass over the stored dx
              float gm = (!bn_relu || bf2f(bn_y[i]) > 0.f) ? bf2f(h) : 0.f;
              bnsb[nr] += gm;
              bnsg[nr] += gm * (bf2f(bn_x[i]) - bnmu[nr]) * bnis[nr];
            }
          }
        }
      }
  if (BNP) {
    // block-reduce the 8 contributors per channel through (repurposed) LDS
    // and write [gy = blockIdx.x][{dgamma, dbeta}][C] partials
    __syncthreads();  // LDS tiles may still be read by slower waves
    float* scr = (float*)lds;  // [2][8][64] floats = 4 KiB
    const int cid = wr * 4 + fi.quad;
#pragma unroll
    for (int nr = 0; nr < 2; ++nr) {
      int cc = wc * 32 + nr * 16 + fi.half;
      scr[(0 * 8 + cid) * 64 + cc] = bnsg[nr];
      scr[(1 * 8 + cid) * 64 + cc] = bnsb[nr];
    }
    __syncthreads();
    if (t < 128) {
      int s = t >> 6, cc = t & 63;
      float a = 0.f;
#pragma unroll
      for (int k8 = 0; k8 < 8; ++k8) a += scr[(s * 8 + k8) * 64 + cc];
      if (c0 + cc < g.C)
        bn_parts[((long)blockIdx.x * 2 + s) * g.C + c0 + cc] = a;
    }
  }
}

// ==================== backward data, stride-2 fused parity ====================
// dX positions partition by (hi%2, wi%2) into 4 classes, each touched by only
// the (r,s) with r = r0+2*jr, s = s0+2*js — one launch, blockIdx.z = class,
// removes the 4x zero-structured MFMA work of the generic strided gather
// without extra launches. Requires stride == 2 and K % 16 == 0 (fast gather).

template <int BKT>
__global__ __launch_bounds__(NTHREADS)
void conv2d_bwd_data_s2_kernel(const bf16_t* __restrict__ dy,
                               const bf16_t* __restrict__ w,
                               bf16_t* __restrict__ dx, ConvGeom g) {
  constexpr int NQ = BKT / 32;
  constexpr int LPX = BKT + 8;
  __shared__ bf16_t lds[2 * BM * LPX + 2 * BN * LPX];
  const int AS0 = 0, BS0 = 2 * BM * LPX;
  const int cls = blockIdx.z;
  const int ph = cls >> 1, pw = cls & 1;
  const int H2 = (g.H - ph + 1) >> 1, W2 = (g.W - pw + 1) >> 1;
  const int r0 = (ph + g.pad) & 1, s0 = (pw + g.pad2) & 1;
  const int nr = (g.R - r0 + 1) >> 1, ns = (g.S - s0 + 1) >> 1;
  const int padh = (ph + g.pad - r0) >> 1, padw = (pw + g.pad2 - s0) >> 1;
  const int Mc = g.N * H2 * W2;
  const int RSK = nr * ns * g.K;
  const int nk = cdiv_i(RSK, BKT);
  const int m0 = blockIdx.x * BM;
  if (m0 >= Mc || nr <= 0 || ns <= 0) return;
  const int c0 = blockIdx.y * BN;
  const int t = threadIdx.x;
  const int wave = t >> 6, wr = wave >> 1, wc = wave & 1;

  const int arow = t >> 1, ahalf = t & 1;
  int m = m0 + arow;
  bool arow_ok = m < Mc;
  int mc_ = min(m, Mc - 1);
  int an = mc_ / (H2 * W2);
  int mrem = mc_ - an * (H2 * W2);
  int ah2 = mrem / W2;
  int aw2 = mrem - ah2 * W2;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  int4 areg[2 * NQ];
  __align__(16) bf16_t breg[NQ][8];

  // incremental (jr, js, kc) decomposition per q-chunk (A and B gathers)
  int inc_jr[NQ], inc_js[NQ], inc_kc[NQ];
  int binc_jr[NQ], binc_js[NQ], binc_kc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    int k = q * 32 + ahalf * 16;  // kt0 == 0 (no ksplit)
    int rs = k / g.K;
    inc_kc[q] = k - rs * g.K;
    inc_jr[q] = rs / ns;
    inc_js[q] = rs - inc_jr[q] * ns;
    int bk = (t & 3) * 8 + q * 32;
    int brs = bk / g.K;
    binc_kc[q] = bk - brs * g.K;
    binc_jr[q] = brs / ns;
    binc_js[q] = brs - binc_jr[q] * ns;
  }

  auto stage_to_regs = [&](int kt) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int kc0 = inc_kc[q], jr = inc_jr[q], js = inc_js[q];
      {
        int ho = ah2 + padh - jr, wo = aw2 + padw - js;
        bool ok = arow_ok & ((unsigned)ho < (unsigned)g.Ho)
                  & ((unsigned)wo < (unsigned)g.Wo);
        int hoc = min(max(ho, 0), g.Ho - 1);
        int woc = min(max(wo, 0), g.Wo - 1);
        const int4* src = (const int4*)&dy[(((long)an * g.Ho + hoc) * g.Wo
                                            + woc) * g.K + kc0];
        areg[2 * q] = masked_i4(src[0], ok);
        areg[2 * q + 1] = masked_i4(src[1], ok);
        kc0 += BKT;
        while (kc0 >= g.K) {
          kc0 -= g.K;
          if (++js == ns) { js = 0; ++jr; }
        }
        inc_kc[q] = kc0; inc_jr[q] = jr; inc_js[q] = js;
      }
      // B: Bs[c][kk] = w[((r0+2jr)*S + s0+2js)*C + c][kc]
      const int bc = t >> 2, bkk = (t & 3) * 8 + q * 32;
      int k = kt * BKT + bkk;
      {
        int kc = binc_kc[q], jr2 = binc_jr[q], js2 = binc_js[q];
        bool ok = (k < RSK) & (c0 + bc < g.C);
        int bcc = min(c0 + bc, g.C - 1);
        int jr2c = min(jr2, nr - 1), js2c = min(js2, ns - 1);
        int rs_orig = (r0 + 2 * jr2c) * g.S + s0 + 2 * js2c;
        const int4* src = (const int4*)&w[((long)rs_orig * g.C + bcc)
                                          * g.K + kc];
        *(int4*)breg[q] = masked_i4(*src, ok);
        kc += BKT;
        while (kc >= g.K) {
          kc -= g.K;
          if (++js2 == ns) { js2 = 0; ++jr2; }
        }
        binc_kc[q] = kc; binc_jr[q] = jr2; binc_js[q] = js2;
      }
    }
  };

  auto regs_to_lds = [&](int buf) {
    bf16_t* As = &lds[AS0 + buf * BM * LPX];
    bf16_t* Bs = &lds[BS0 + buf * BN * LPX];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      *(int4*)&As[arow * LPX + q * 32 + ahalf * 16] = areg[2 * q];
      *(int4*)&As[arow * LPX + q * 32 + ahalf * 16 + 8] = areg[2 * q + 1];
      const int bc = t >> 2, bkk = (t & 3) * 8 + q * 32;
      *(int4*)&Bs[bc * LPX + bkk] = *(int4*)breg[q];
    }
  };

  stage_to_regs(0);
  regs_to_lds(0);
  __syncthreads();
  FragIdx fi = frag_idx();
  for (int kt = 0; kt < nk; ++kt) {
    int cur = kt & 1;
    if (kt + 1 < nk) stage_to_regs(kt + 1);
    {
      const bf16_t* As = &lds[AS0 + cur * BM * LPX];
      const bf16_t* Bs = &lds[BS0 + cur * BN * LPX];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int kb = fi.quad * 8 + q * 32;
#pragma unroll
        for (int mr = 0; mr < 4; ++mr) {
          int row = wr * 64 + mr * 16 + fi.half;
          bf16x8 a = *(const bf16x8*)&As[row * LPX + kb];
#pragma unroll
          for (int nrr = 0; nrr < 2; ++nrr) {
            int col = wc * 32 + nrr * 16 + fi.half;
            bf16x8 b = *(const bf16x8*)&Bs[col * LPX + kb];
            acc[mr][nrr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b, acc[mr][nrr], 0, 0, 0);
          }
        }
      }
    }
    if (kt + 1 < nk) {
      regs_to_lds(cur ^ 1);
      __syncthreads();
    }
  }

#pragma unroll
  for (int mr = 0; mr < 4; ++mr)
#pragma unroll
    for (int nrr = 0; nrr < 2; ++nrr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mr * 16 + fi.quad * 4 + r;
        int col = c0 + wc * 32 + nrr * 16 + fi.half;
        if (row < Mc && col < g.C) {
          int n = row / (H2 * W2);
          int rem = row - n * (H2 * W2);
          int h2 = rem / W2, w2 = rem - h2 * W2;
          dx[(((long)n * g.H + ph + 2 * h2) * g.W + pw + 2 * w2) * g.C + col]
              = f2bf(acc[mr][nrr][r]);
        }
      }
}

// ============================== backward weight ==============================
// dW[(r,s,c), k] = sum_m X[m -> (n,hi,wi,c)] * dY[m, k]; the m-reduction is
// split over blockIdx.z into fp32 partial slabs (reduced by reduce_slabs_f32).
// Tile 64(CRS) x 64(K) x 64(m) — BK=64 halves barrier count vs the conv tiles.

#define WBM 64
#define WBK 64
// LDS images are [rowgrp(4)][m(64)][16] per operand — m-major within a
// 16-row column group (32 B m-stride, the attention-V tr-read shape): the
// gather's natural int4 (8 rows of one m) lands as ONE b128 write, and the
// MFMA fragment (one row, 8 m's) comes back as TWO ds_read_b64_tr_b16.
// Replaces the round-1 [row][m] image whose transpose staging was 32 scalar
// ds_write_b16 per thread per K-step (the biggest measured kernel cost).
// +16-elem pad between 16-col groups: staging's 8 write lanes then start at
// 8 distinct 4-dword bank ranges (conflict-free ds_write_b128)
#define WGRP_ELEMS (WBK * 16 + 16)
#define WIMG_ELEMS (4 * WGRP_ELEMS)      // one operand image (64 rows)
#define WAS_OFF(buf) ((buf) * WIMG_ELEMS)
#define WBS_OFF(buf) (2 * WIMG_ELEMS + (buf) * WIMG_ELEMS)
#define WLDS_ELEMS (4 * WIMG_ELEMS)

// two transpose-reads -> one MFMA operand fragment.
// Measured gfx950 semantics (tools/probe/trprobe.hip): each lane loads 8
// ALIGNED bytes at its own address; per 16-lane group, "row" j is the 32 B
// loaded by lanes 4j..4j+3 and lane s receives element s of each row. So
// with lane address = img + (mbase + ((l>>2)&3))*32B + (l&3)*8B over a
// [m][16 col] image, lane s = l&15 gets col s at m = mbase+j — one MFMA
// operand column slice; the offset:128 twin covers m = mbase+4..7.
DEV bf16x8 tr_frag(unsigned lds_byte) {
  typedef __attribute__((ext_vector_type(4))) short s4;
  s4 lo, hi;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:128\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo), "=&v"(hi)
      : "v"(lds_byte));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <bool FAST>
__global__ __launch_bounds__(NTHREADS)
void conv2d_bwd_weight_kernel(const bf16_t* __restrict__ dy,
                              const bf16_t* __restrict__ x,
                              float* __restrict__ ws, ConvGeom g, int M,
                              int CRS, int slice_len) {
  __shared__ bf16_t lds[WLDS_ELEMS];
  const int rs0 = blockIdx.x * WBM;
  const int ko0 = blockIdx.y * BN;
  const int ms = blockIdx.z * slice_len;
  const int me = min(ms + slice_len, M);
  const int t = threadIdx.x;
  const int wave = t >> 6, wr = wave >> 1, wc = wave & 1;

  const int amm = t >> 3, agrp = t & 7;
  const int rowb = rs0 + agrp * 8;
  bool agrp_ok = rowb < CRS;
  // clamp to the last 8-aligned chunk (FAST: C%8==0 => CRS%8==0), so the
  // int4 gather of a clamped row stays 8-aligned and inside the pixel row
  const int rowbc = min(rowb, max(CRS - 8, 0));
  int rs_ = rowbc / g.C;
  int cbase_ = rowbc - rs_ * g.C;
  int r_ = rs_ / g.S;
  int s_ = rs_ - r_ * g.S;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  __align__(16) bf16_t areg[2][8];
  __align__(16) bf16_t breg[2][8];
  const int HoWo = g.Ho * g.Wo;

  const bool flat = (g.H == 1 && g.W == 1 && g.Ho == 1 && g.Wo == 1);
  auto gather_one = [&](int m, bf16_t* adst, bf16_t* bdst) {
    const bool m_ok = m < me;
    const int mcl = min(m, me - 1);
    int n, ho = 0, wo = 0;
    if (!flat) {  // wave-uniform condition; magic division (hot loop)
      n = (int)mdiv40((unsigned)mcl, g.m_howo);
      int rem = mcl - n * HoWo;
      ho = (int)mdiv40((unsigned)rem, g.m_wo);
      wo = rem - ho * g.Wo;
    } else {
      n = mcl;  // flat im2col geometry: one "pixel" per row
    }
    if (FAST) {
      int hi = ho * g.stride - g.pad + r_;
      int wi = wo * g.stride - g.pad2 + s_;
      bool ok = agrp_ok & m_ok & ((unsigned)hi < (unsigned)g.H)
                & ((unsigned)wi < (unsigned)g.W);
      int hic = min(max(hi, 0), g.H - 1);
      int wic = min(max(wi, 0), g.W - 1);
      *(int4*)adst = masked_i4(*(const int4*)&x[(((long)n * g.H + hic) * g.W
                                                 + wic) * g.C + cbase_], ok);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int row = rowb + j;
        int rowc = min(row, CRS - 1);
        int rs = (int)mdiv40((unsigned)rowc, g.m_ck);
        int c = rowc - rs * g.C;
        int r = (int)mdiv40((unsigned)rs, g.m_s);
        int s = rs - r * g.S;
        int hi = ho * g.stride - g.pad + r;
        int wi = wo * g.stride - g.pad2 + s;
        bool ok = (row < CRS) & m_ok & ((unsigned)hi < (unsigned)g.H)
                  & ((unsigned)wi < (unsigned)g.W);
        int hic = min(max(hi, 0), g.H - 1);
        int wic = min(max(wi, 0), g.W - 1);
        bf16_t v = x[(((long)n * g.H + hic) * g.W + wic) * g.C + c];
        adst[j] = ok ? v : (bf16_t)0;
      }
    }
    if (ko0 + BN <= g.K) {  // block-uniform: full 64-col dY tile
      *(int4*)bdst = masked_i4(
          *(const int4*)&dy[(long)mcl * g.K + ko0 + agrp * 8], m_ok);
    } else if (m_ok) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        bdst[j] = (ko0 + agrp * 8 + j < g.K)
                      ? dy[(long)m * g.K + ko0 + agrp * 8 + j] : 0;
    } else {
      *(int4*)bdst = int4{0, 0, 0, 0};
    }
  };

  auto stage_to_regs = [&](int m0) {
    gather_one(m0 + amm, areg[0], breg[0]);
    gather_one(m0 + amm + 32, areg[1], breg[1]);
  };

  auto regs_to_lds = [&](int buf) {
    // one b128 write per gather: image[rowgrp][m][16], rowgrp = agrp>>1,
    // in-group column base = (agrp&1)*8
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = (agrp >> 1) * WGRP_ELEMS + (amm + h * 32) * 16
                    + (agrp & 1) * 8;
      *(int4*)&lds[WAS_OFF(buf) + e] = *(int4*)areg[h];
      *(int4*)&lds[WBS_OFF(buf) + e] = *(int4*)breg[h];
    }
  };

  const int nk = cdiv_i(me - ms, WBK);
  if (nk > 0) {
    stage_to_regs(ms);
    regs_to_lds(0);
  }
  __syncthreads();
  FragIdx fi = frag_idx();
  // per-lane tr-read byte bases: lane covers m-row (fi.quad*8 + ((l>>2)&3)),
  // byte slot (l&3)*8 of the 32 B row; received = col (l&15), m quad*8+j
  const unsigned lds0 = (unsigned)(uintptr_t)&lds[0];
  const int lane = t & 63;
  const unsigned lane_e = (unsigned)((fi.quad * 8 + ((lane >> 2) & 3)) * 16
                                     + (lane & 3) * 4);
  for (int kt = 0; kt < nk; ++kt) {
    int cur = kt & 1;
    if (kt + 1 < nk) stage_to_regs(ms + (kt + 1) * WBK);
    {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const unsigned khe = lane_e + kh * 32 * 16;
        bf16x8 a0 = tr_frag(lds0 + 2 * (WAS_OFF(cur)
                            + (wr * 2 + 0) * WGRP_ELEMS + khe));
        bf16x8 a1 = tr_frag(lds0 + 2 * (WAS_OFF(cur)
                            + (wr * 2 + 1) * WGRP_ELEMS + khe));
        bf16x8 b0 = tr_frag(lds0 + 2 * (WBS_OFF(cur)
                            + (wc * 2 + 0) * WGRP_ELEMS + khe));
        bf16x8 b1 = tr_frag(lds0 + 2 * (WBS_OFF(cur)
                            + (wc * 2 + 1) * WGRP_ELEMS + khe));
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0,
                                                            acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1,
                                                            acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0,
                                                            acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1,
                                                            acc[1][1], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) {  // single barrier per K-step (see fwd kernel note)
      regs_to_lds(cur ^ 1);
      __syncthreads();
    }
  }

  const long slab = (long)blockIdx.z * CRS * g.K;
#pragma unroll
  for (int mr = 0; mr < 2; ++mr)
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = rs0 + wr * 32 + mr * 16 + fi.quad * 4 + r;
        int col = ko0 + wc * 32 + nr * 16 + fi.half;
        if (row < CRS && col < g.K)
          ws[slab + (long)row * g.K + col] = acc[mr][nr][r];
      }
}

// tiny-C (stem) im2col: col (M, CRSpad) bf16, one thread per (m, r*S+s)
// copying the C input channels; OOB pixels stay zero (buffer pre-zeroed).
// Pixel decomposition comes from the packed mt table.
__global__ __launch_bounds__(NTHREADS)
void im2col_smallc_kernel(const bf16_t* __restrict__ x,
                          const int* __restrict__ mt,
                          bf16_t* __restrict__ col, ConvGeom g, int M,
                          int CRSpad, long total) {
  long i = (long)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int RS = g.R * g.S;
  int rs = (int)(i % RS);
  int m = (int)(i / RS);
  const int v = mt[m];
  const int n = v >> 20;
  const int r = rs / g.S, s = rs - (rs / g.S) * g.S;
  const int hi = ((v >> 10) & 1023) - g.pad + r;
  const int wi = (v & 1023) - g.pad2 + s;
  if (hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return;
  const bf16_t* src = &x[(((long)n * g.H + hi) * g.W + wi) * g.C];
  bf16_t* dst = &col[(long)m * CRSpad + rs * g.C];
  for (int c = 0; c < g.C; ++c) dst[c] = src[c];
}

// packed im2col pixel table: mt[m] = n<<20 | (ho*stride)<<10 | (wo*stride)
__global__ __launch_bounds__(NTHREADS)
void fill_mtable_kernel(int* __restrict__ mt, int M, int HoWo, int Wo,
                        int stride) {
  int m = blockIdx.x * NTHREADS + threadIdx.x;
  if (m >= M) return;
  int n = m / HoWo;
  int rem = m - n * HoWo;
  int ho = rem / Wo;
  int wo = rem - ho * Wo;
  mt[m] = (n << 20) | ((ho * stride) << 10) | (wo * stride);
}


// ========================= forward v2 (all-glds) =========================
// 2-phase all-global_load_lds staging (guide T3 minimum 2-phase + the glds
// rows of the staging table): the A tile's gather sources are PER-LANE glds
// addresses (a zero page absorbs OOB lanes), XOR-swizzled at the source so
// the linear LDS image reads conflict-free; the B tile lands as [ngrp][k][16]
// images consumed by ds_read_b64_tr_b16 pairs (w is k-major — glds cannot
// transpose). One raw barrier + vmcnt(0) per K-step, whole-phase setprio.
// Requires C % 8 == 0 (an 8-elem chunk stays inside one (r,s)).
// Measured (tools/probe/convfwd_v2.hip): l1 337 TF, l2 375, l3 257 vs the
// register-staged v1's 274/261/219; 3-buffer counted-vmcnt was null at this
// occupancy (3 blocks/CU), BM=256 and BKT=64-everywhere lose to occupancy.

#define V2BK 64
#define V2_A_ELEMS (BM * V2BK)
#define V2_B_ELEMS (4 * V2BK * 16)
#define V2_BUF (V2_A_ELEMS + V2_B_ELEMS)

template <int BNX2 = BN>
__global__ __launch_bounds__(NTHREADS)
void conv2d_fwd_v2_kernel(const bf16_t* __restrict__ x,
                          const bf16_t* __restrict__ w,
                          bf16_t* __restrict__ y, float* __restrict__ ws,
                          const bf16_t* __restrict__ zpage, ConvGeom g,
                          int M, int CRS, int nk, int ksplit,
                          float* __restrict__ bn_parts) {
  constexpr int NGRP = BNX2 / 16;       // 16-col groups in the B tile
  constexpr int NRC = BNX2 / 32;        // N-fragments per wave
  constexpr int BEL = NGRP * V2BK * 16; // B image elems
  constexpr int BUFE = V2_A_ELEMS + BEL;
  __shared__ bf16_t lds[2 * BUFE];
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BNX2;
  const int t = threadIdx.x;
  const int wv = t >> 6, lane = t & 63;
  const int wr = wv >> 1, wc = wv & 1;
  const int steps = (nk + ksplit - 1) / ksplit;
  const int kt0 = blockIdx.z * steps;
  const int kt1 = min(kt0 + steps, nk);
  const int nsteps = kt1 - kt0;

  // A staging: 16 glds x 8 rows; wave wv does instrs wv*4..+3. Lane covers
  // row wv*32 + i*8 + l/8, source k-chunk (l%8) ^ (row&7) (source swizzle).
  int achunk[4], ar[4], as_[4], ac[4];
  bool mok[4];
  int an[4], ahb[4], awb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int row = wv * 32 + i * 8 + (lane >> 3);
    achunk[i] = (lane & 7) ^ (row & 7);
    int m = m0 + row;
    mok[i] = m < M;
    int mc = min(m, M - 1);
    int n = mc / (g.Ho * g.Wo);
    int rem = mc - n * (g.Ho * g.Wo);
    int aho = rem / g.Wo;
    an[i] = n;
    ahb[i] = aho * g.stride - g.pad;
    awb[i] = (rem - aho * g.Wo) * g.stride - g.pad2;
    int k = kt0 * V2BK + achunk[i] * 8;
    int rs = k / g.C;
    ac[i] = k - rs * g.C;
    ar[i] = rs / g.S;
    as_[i] = rs - ar[i] * g.S;
  }
  // B staging: 2 glds per wave into [ngrp=wv][k][16]
  const int bk0 = lane >> 1;
  const int bns = (lane & 1) * 8;

  f32x4 acc[4][NRC];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NRC; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  auto stage = [&](int buf, int kt) {
    bf16_t* base = &lds[buf * BUFE];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int hi = ahb[i] + ar[i], wi = awb[i] + as_[i];
      int k = kt * V2BK + achunk[i] * 8;
      bool ok = mok[i] & (k < CRS) & ((unsigned)hi < (unsigned)g.H)
                & ((unsigned)wi < (unsigned)g.W);
      const bf16_t* src = ok
          ? &x[(((long)an[i] * g.H + hi) * g.W + wi) * g.C + ac[i]]
          : zpage;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)
              &base[(wv * 4 + i) * 8 * V2BK], 16, 0, 0);
      int c = ac[i] + V2BK;
      int r = ar[i], s = as_[i];
      while (c >= g.C) { c -= g.C; if (++s == g.S) { s = 0; ++r; } }
      ac[i] = c; ar[i] = r; as_[i] = s;
    }
    // B: (NGRP/4) groups per wave x 2 glds each
#pragma unroll
    for (int gset = 0; gset < NGRP / 4; ++gset) {
      const int ng = wv + gset * 4;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int k = kt * V2BK + j * 32 + bk0;
        int kc = min(k, CRS - 1);
        bool ok = (k < CRS) & (n0 + ng * 16 + bns + 8 <= g.K);
        const bf16_t* src = ok ? &w[(long)kc * g.K + n0 + ng * 16 + bns]
                               : zpage;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)src,
            (__attribute__((address_space(3))) unsigned int*)
                &base[V2_A_ELEMS + ng * (V2BK * 16) + j * 32 * 16],
            16, 0, 0);
      }
    }
  };

  const int fh = lane & 15, fq = lane >> 4;
  const unsigned lds0 = (unsigned)(uintptr_t)&lds[0];
  const unsigned btr_e = (unsigned)((fq * 8 + ((lane >> 2) & 3)) * 16
                                    + (lane & 3) * 4);

  if (nsteps > 0) stage(0, kt0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int kt = kt0; kt < kt1; ++kt) {
    int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) stage(cur ^ 1, kt + 1);
    const bf16_t* As = &lds[cur * BUFE];
    const unsigned bbase = lds0 + 2u * (cur * BUFE + V2_A_ELEMS);
    bf16x8 bfr[2][NRC];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int nr = 0; nr < NRC; ++nr) {
        unsigned a = bbase + 2u * ((wc * NRC + nr) * (V2BK * 16))
                     + 2u * (btr_e + q * 32 * 16);
        typedef __attribute__((ext_vector_type(4))) short s4_t;
        s4_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                     "ds_read_b64_tr_b16 %1, %2 offset:128\n\t"
                     : "=&v"(lo), "=&v"(hi) : "v"(a));
        bfr[q][nr] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int kb = fq * 8 + q * 32;
#pragma unroll
      for (int mr = 0; mr < 4; ++mr) {
        int row = wr * 64 + mr * 16 + fh;
        int kcol = kb ^ ((row & 7) << 3);
        bf16x8 afr = *(const bf16x8*)&As[row * V2BK + kcol];
        if (q == 0 && mr == 0) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
        }
#pragma unroll
        for (int nr = 0; nr < NRC; ++nr)
          acc[mr][nr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr, bfr[q][nr], acc[mr][nr], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

#pragma unroll
  for (int mr = 0; mr < 4; ++mr)
#pragma unroll
    for (int nr = 0; nr < NRC; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mr * 16 + fq * 4 + r;
        int col = n0 + wc * (16 * NRC) + nr * 16 + fh;
        if (row < M && col < g.K) {
          if (ksplit > 1)
            ws[((long)blockIdx.z * M + row) * g.K + col] = acc[mr][nr][r];
          else
            y[(long)row * g.K + col] = f2bf(acc[mr][nr][r]);
        }
      }

  // fused BN partial sums (a following training BN consumes these instead
  // of re-reading y in its own bn_sums pass): per-column sum / sum-of-
  // squares over this block's VALID rows, deterministic fixed-order
  // reduce through the (reused) staging LDS, one [2][K] row per M-block.
  if (bn_parts != nullptr) {
    __syncthreads();
    float* red = (float*)lds;  // [4 wv][4 fq][BNX2][2] = 16 KB max
#pragma unroll
    for (int nr = 0; nr < NRC; ++nr) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int mr = 0; mr < 4; ++mr)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = m0 + wr * 64 + mr * 16 + fq * 4 + r;
          // match the stored activation: the BN input is the bf16 y
          float v = (row < M) ? bf2f(f2bf(acc[mr][nr][r])) : 0.f;
          s1 += v;
          s2 += v * v;
        }
      int cl = wc * (16 * NRC) + nr * 16 + fh;
      red[((wv * 4 + fq) * BNX2 + cl) * 2] = s1;
      red[((wv * 4 + fq) * BNX2 + cl) * 2 + 1] = s2;
    }
    __syncthreads();
    // 2*BNX2 (col, quantity) entries; sum the 8 slots that own the col
    for (int e = t; e < 2 * BNX2; e += NTHREADS) {
      int cl = e >> 1, qi = e & 1;
      int wcc = cl / (16 * NRC);
      float a = 0.f;
#pragma unroll
      for (int wrr = 0; wrr < 2; ++wrr)
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2)
          a += red[(((wrr * 2 + wcc) * 4 + q2) * BNX2 + cl) * 2 + qi];
      int col = n0 + cl;
      if (col < g.K)
        bn_parts[((long)blockIdx.x * 2 + qi) * g.K + col] = a;
    }
  }
}


// ==================== backward data v2 (all-glds) ====================
// Same 2-phase all-glds structure as fwd v2. A = scattered dY gather
// (stride handled by shift-select + parity mask); B = W consumed as
// [c][rsk] — for a fixed channel c, consecutive kc are CONTIGUOUS in the
// (R,S,C,K) weight layout, so B stages through plain per-lane glds with
// the same XOR source swizzle as A and fragments read as b128 (no
// transpose read needed, unlike fwd's B). Requires K % 8 == 0.

__global__ __launch_bounds__(NTHREADS)
void conv2d_bwd_data_v2_kernel(const bf16_t* __restrict__ dy,
                               const bf16_t* __restrict__ w,
                               bf16_t* __restrict__ dx,
                               float* __restrict__ ws,
                               const bf16_t* __restrict__ zpage, ConvGeom g,
                               int M, int RSK, int nk, int ksplit) {
  __shared__ bf16_t lds[2 * (BM * V2BK + BN * V2BK)];
  const int A_E = BM * V2BK;
  const int BUF = BM * V2BK + BN * V2BK;
  const int m0 = blockIdx.x * BM;
  const int c0 = blockIdx.y * BN;
  const int t = threadIdx.x;
  const int wv = t >> 6, lane = t & 63;
  const int wr = wv >> 1, wc = wv & 1;
  const int steps = (nk + ksplit - 1) / ksplit;
  const int kt0 = blockIdx.z * steps;
  const int kt1 = min(kt0 + steps, nk);

  // A: 16 glds x 8 rows of the [128][64] dY-gather image
  int achunk[4], ar[4], as_[4], akc[4];
  bool mok[4];
  int an[4], ahi[4], awi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int row = wv * 32 + i * 8 + (lane >> 3);
    achunk[i] = (lane & 7) ^ (row & 7);
    int m = m0 + row;
    mok[i] = m < M;
    int mc = min(m, M - 1);
    an[i] = mc / (g.H * g.W);
    int rem = mc - an[i] * (g.H * g.W);
    ahi[i] = rem / g.W;
    awi[i] = rem - ahi[i] * g.W;
    int k = kt0 * V2BK + achunk[i] * 8;
    int rs = k / g.K;
    akc[i] = k - rs * g.K;
    ar[i] = rs / g.S;
    as_[i] = rs - ar[i] * g.S;
  }
  // B: 8 glds (2/wave) into the [64 c][64 rsk] image, source swizzled
  int bchunk[2], br[2], bs_[2], bkc[2], brow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    brow[j] = wv * 16 + j * 8 + (lane >> 3);
    bchunk[j] = (lane & 7) ^ (brow[j] & 7);
    int k = kt0 * V2BK + bchunk[j] * 8;
    int rs = k / g.K;
    bkc[j] = k - rs * g.K;
    br[j] = rs / g.S;
    bs_[j] = rs - br[j] * g.S;
  }

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[i][0] = f32x4{0, 0, 0, 0};
    acc[i][1] = f32x4{0, 0, 0, 0};
  }
  const bool s2d = g.stride == 2;

  auto stage = [&](int buf, int kt) {
    bf16_t* base = &lds[buf * BUF];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int k = kt * V2BK + achunk[i] * 8;
      int ho2 = ahi[i] + g.pad - ar[i], wo2 = awi[i] + g.pad2 - as_[i];
      int ho = s2d ? (ho2 >> 1) : ho2;
      int wo = s2d ? (wo2 >> 1) : wo2;
      bool par = !s2d | (((ho2 | wo2) & 1) == 0);
      bool ok = mok[i] & (k < RSK) & (ho2 >= 0) & (wo2 >= 0) & par
                & (ho < g.Ho) & (wo < g.Wo);
      const bf16_t* src = ok
          ? &dy[(((long)an[i] * g.Ho + ho) * g.Wo + wo) * g.K + akc[i]]
          : zpage;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)
              &base[(wv * 4 + i) * 8 * V2BK], 16, 0, 0);
      int kc = akc[i] + V2BK;
      int r = ar[i], s = as_[i];
      while (kc >= g.K) { kc -= g.K; if (++s == g.S) { s = 0; ++r; } }
      akc[i] = kc; ar[i] = r; as_[i] = s;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int k = kt * V2BK + bchunk[j] * 8;
      int rs_orig = br[j] * g.S + bs_[j];
      bool ok = (k < RSK) & (c0 + brow[j] < g.C) & (rs_orig < g.R * g.S);
      const bf16_t* src = ok
          ? &w[((long)rs_orig * g.C + c0 + brow[j]) * g.K + bkc[j]]
          : zpage;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)
              &base[A_E + (wv * 2 + j) * 8 * V2BK], 16, 0, 0);
      int kc = bkc[j] + V2BK;
      int r = br[j], s = bs_[j];
      while (kc >= g.K) { kc -= g.K; if (++s == g.S) { s = 0; ++r; } }
      bkc[j] = kc; br[j] = r; bs_[j] = s;
    }
  };

  const int fh = lane & 15, fq = lane >> 4;

  if (kt1 > kt0) stage(0, kt0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int kt = kt0; kt < kt1; ++kt) {
    int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) stage(cur ^ 1, kt + 1);
    const bf16_t* As = &lds[cur * BUF];
    const bf16_t* Bs = &lds[cur * BUF + A_E];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int kb = fq * 8 + q * 32;
#pragma unroll
      for (int mr = 0; mr < 4; ++mr) {
        int row = wr * 64 + mr * 16 + fh;
        bf16x8 afr = *(const bf16x8*)&As[row * V2BK
                                         + (kb ^ ((row & 7) << 3))];
        if (q == 0 && mr == 0) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int nr = 0; nr < 2; ++nr) {
          int col = wc * 32 + nr * 16 + fh;
          bf16x8 bfr = *(const bf16x8*)&Bs[col * V2BK
                                           + (kb ^ ((col & 7) << 3))];
          acc[mr][nr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr, bfr, acc[mr][nr], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

#pragma unroll
  for (int mr = 0; mr < 4; ++mr)
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mr * 16 + fq * 4 + r;
        int col = c0 + wc * 32 + nr * 16 + fh;
        if (row < M && col < g.C) {
          if (ksplit > 1)
            ws[((long)blockIdx.z * M + row) * g.C + col] = acc[mr][nr][r];
          else
            dx[(long)row * g.C + col] = f2bf(acc[mr][nr][r]);
        }
      }
}


// ==================== backward weight v2 (all-glds) ====================
// dW[(r,s,c), k] = sum_m X-gather[m] * dY[m]: BOTH operands are m-major at
// the source (x: 16 B = 8 CRS rows of one pixel; dy: 16 B = 8 K of one m),
// exactly the [grp][m][16] tr_b16 image shape — so both stage by
// global_load_lds (no register round-trip, no ds_write pass) and fragments
// come back as ds_read_b64_tr_b16 pairs. 2-phase raw-barrier loop like
// fwd v2. Requires C % 8 == 0 and K % 8 == 0.

#define W2_IMG (4 * WBK * 16)   // one operand image: [4 grp][64 m][16]

__global__ __launch_bounds__(NTHREADS)
void conv2d_bwd_weight_v2_kernel(const bf16_t* __restrict__ dy,
                                 const bf16_t* __restrict__ x,
                                 float* __restrict__ ws,
                                 const bf16_t* __restrict__ zpage,
                                 ConvGeom g, int M, int CRS, int slice_len) {
  __shared__ bf16_t lds[2 * 2 * W2_IMG];
  const int rs0 = blockIdx.x * WBM;
  const int ko0 = blockIdx.y * BN;
  const int ms = blockIdx.z * slice_len;
  const int me = min(ms + slice_len, M);
  const int t = threadIdx.x;
  const int wv = t >> 6, lane = t & 63;
  const int wr = wv >> 1, wc = wv & 1;
  const int HoWo = g.Ho * g.Wo;
  const bool flat = (g.H == 1 && g.W == 1 && g.Ho == 1 && g.Wo == 1);

  // lane's m within the 64-m tile and its 8-row chunk: 4 glds per wave per
  // operand; instr i covers m rows [i*16, i*16+16), lane -> m = i*16 + l/4,
  // chunk = l%4 is WRONG for 16-wide rows: [64 m][16] rows are 32 B = 2
  // lanes -> lane covers m = i*32 + l/2, half = l&1 (8 elems).
  // A (x-gather): CRS rows grp*16 + (l&1)*8 .. +8 of pixel m.
  const int lm = lane >> 1;         // m offset within a 32-m slab
  const int lh = lane & 1;          // which 8-row half of the 16-wide row
  // per-wave A group = wv; crs row base for this lane:
  const int acrs = rs0 + wv * 16 + lh * 8;
  const bool aok_row = acrs < CRS;
  const int acrsc = min(acrs, max(CRS - 8, 0));
  int ars = acrsc / g.C;
  const int ac = acrsc - ars * g.C;
  const int ar = ars / g.S;
  const int as_ = ars - ar * g.S;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    acc[i][0] = f32x4{0, 0, 0, 0};
    acc[i][1] = f32x4{0, 0, 0, 0};
  }

  auto stage = [&](int buf, int m0) {
    bf16_t* base = &lds[buf * 2 * W2_IMG];
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // two 32-m slabs per 64-m tile
      int m = m0 + i * 32 + lm;
      bool m_ok = m < me;
      int mcl = min(m, me - 1);
      int n, ho = 0, wo = 0;
      if (!flat) {
        n = (int)mdiv40((unsigned)mcl, g.m_howo);
        int rem = mcl - n * HoWo;
        ho = (int)mdiv40((unsigned)rem, g.m_wo);
        wo = rem - ho * g.Wo;
      } else {
        n = mcl;
      }
      int hi = ho * g.stride - g.pad + ar;
      int wi = wo * g.stride - g.pad2 + as_;
      bool ok = aok_row & m_ok & ((unsigned)hi < (unsigned)g.H)
                & ((unsigned)wi < (unsigned)g.W);
      const bf16_t* srcA = ok
          ? &x[(((long)n * g.H + hi) * g.W + wi) * g.C + ac]
          : zpage;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcA,
          (__attribute__((address_space(3))) unsigned int*)
              &base[wv * (WBK * 16) + i * 32 * 16], 16, 0, 0);
      // B: dy[m][ko0 + wv*16 + lh*8 .. +8]
      bool bok = m_ok & (ko0 + wv * 16 + lh * 8 + 8 <= g.K);
      const bf16_t* srcB = bok
          ? &dy[(long)mcl * g.K + ko0 + wv * 16 + lh * 8]
          : zpage;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcB,
          (__attribute__((address_space(3))) unsigned int*)
              &base[W2_IMG + wv * (WBK * 16) + i * 32 * 16], 16, 0, 0);
    }
  };

  const int fh = lane & 15, fq = lane >> 4;
  const unsigned lds0 = (unsigned)(uintptr_t)&lds[0];
  const unsigned tr_e = (unsigned)((fq * 8 + ((lane >> 2) & 3)) * 16
                                   + (lane & 3) * 4);

  const int nk = cdiv_i(me - ms, WBK);
  if (nk > 0) stage(0, ms);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int kt = 0; kt < nk; ++kt) {
    int cur = kt & 1;
    if (kt + 1 < nk) stage(cur ^ 1, ms + (kt + 1) * WBK);
    const unsigned abase = lds0 + 2u * (cur * 2 * W2_IMG);
    const unsigned bbase = abase + 2u * W2_IMG;
    typedef __attribute__((ext_vector_type(4))) short s4_t;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const unsigned khe = 2u * (tr_e + kh * 32 * 16);
      bf16x8 afr[2], bfr[2];
#pragma unroll
      for (int mr = 0; mr < 2; ++mr) {
        unsigned a = abase + 2u * ((wr * 2 + mr) * (WBK * 16)) + khe;
        s4_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                     "ds_read_b64_tr_b16 %1, %2 offset:128\n\t"
                     : "=&v"(lo), "=&v"(hi) : "v"(a));
        afr[mr] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int nr = 0; nr < 2; ++nr) {
        unsigned a = bbase + 2u * ((wc * 2 + nr) * (WBK * 16)) + khe;
        s4_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                     "ds_read_b64_tr_b16 %1, %2 offset:128\n\t"
                     : "=&v"(lo), "=&v"(hi) : "v"(a));
        bfr[nr] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      if (kh == 0) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mr = 0; mr < 2; ++mr)
#pragma unroll
        for (int nr = 0; nr < 2; ++nr)
          acc[mr][nr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr[mr], bfr[nr], acc[mr][nr], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  const long slab = (long)blockIdx.z * CRS * g.K;
#pragma unroll
  for (int mr = 0; mr < 2; ++mr)
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = rs0 + wr * 32 + mr * 16 + fq * 4 + r;
        int col = ko0 + wc * 32 + nr * 16 + fh;
        if (row < CRS && col < g.K)
          ws[slab + (long)row * g.K + col] = acc[mr][nr][r];
      }
}

// ============================== launchers ==============================

#include <stdio.h>

// ------------------------------------------------------- environment knobs
// docs/knobs.md. Each is read once per process; a knob's special values are
// mapped right where it is read.
#define KNOB_NEVER (1 << 30)

// BKT=64 halves barriers but its 55 KB LDS halves occupancy (2 vs 4 blocks/CU)
// — the crossover is empirical, so the threshold is runtime-tunable.
static int bk64_min_crs() {
  static const int v = env_int("CILFW_CONV_BK64_MIN", 512);
  return v > 0 ? v : KNOB_NEVER;  // 0 disables BKT=64
}

// above this many blocks, BKT=32's higher occupancy wins
static int bk64_max_blocks() {
  static const int v = env_int("CILFW_CONV_BK64_MAXBLOCKS", 768);
  return v;
}

static int ksplit_target() {
  static const int v = env_int("CILFW_CONV_KSPLIT_TARGET", 512);
  return v;
}

static int dw_target() {  // swept 256-2048: 1024 best (41.3k bench)
  static const int v = env_int("CILFW_CONV_DW_TARGET", 1024);
  return v;
}

static int conv_v2_enabled() {
  static const int v = env_int("CILFW_CONV_V2", 1);
  return v;
}

// bwd-data v2 measured slower than v1 on the CIFAR shapes (l1 pair 129 vs
// 126 us, l3 139 vs 126) but ahead on the large-M ImageNet layers; route by
// M with an env override (CILFW_CONV_V2_BWD_MINM, 0 disables).
static int conv_v2_bwd_minm() {
  static const int v = env_int("CILFW_CONV_V2_BWD_MINM", 150000);
  return v == 0 ? KNOB_NEVER : v;
}

// measured: BM=256 loses to BM=128's occupancy at every ResNet shape — off
// (0) by default
static int fwd_bm256_min_m() {
  static const int v = env_int("CILFW_CONV_BM256_MIN", 0);
  return v > 0 ? v : KNOB_NEVER;
}

// A 128-wide v2 N-tile (2x the MFMA per staged A-byte at 2 blocks/CU) for
// K >= 128 when the grid still fills the chip; 0 turns it off.
static int v2_bn128_enabled() {
  static const int v = env_int("CILFW_CONV_V2_BN128", 1);
  return v;
}

// BN=128 wins only where the A-gather is trivial (1x1 convs: rn50_1x1
// 173->218 TF); on the CIFAR 3x3 layers the halved occupancy loses
// (l2 348->318 at M=32768) — this knob opens the tile to 3x3 layers at/above
// that M (experiment; default -1 = never)
static int v2_bn128_min3x3() {
  static const int v = env_int("CILFW_CONV_V2_BN128_MIN3X3", -1);
  return v >= 0 ? v : KNOB_NEVER;
}

static int s2_fused_enabled() {  // presence-only: any value disables
  static const int v = !env_set("CILFW_NO_S2_FUSED");
  return v;
}

// measured OFF-better on both rn18-CIFAR (41.2k vs 40.6k imgs/s) and
// rn50@224 (4.57k vs 4.55k): the epilogue's two per-element scalar bf16
// reads (mask y + BN input x, column-strided against the acc layout) cost
// more inside the critical-path MFMA kernel than the standalone
// (fully-vectorized) bn_bwd_sums pass they replace. Kept env-gated.
static int bnbwd_fuse_enabled() {
  static const int v = env_int("CILFW_BNBWD_FUSE", 0);
  return v;
}

static int pick_ksplit(int nblocks, int nk) {
  // aim for >= target workgroups without shredding the K loop
  int ks = 1;
  while (ks < 8 && nblocks * ks < ksplit_target() && nk / (ks * 2) >= 4)
    ks *= 2;
  return ks;
}

// ----------------------------------------------------------- slab reduce
static dim3 reduce_slabs_grid(long len) {
  return dim3((unsigned)((len + NTHREADS * 4 - 1) / (NTHREADS * 4)));
}

// split-K epilogue: sums the fp32 slabs into the bf16 output. With
// ksplit == 1 the MFMA kernel stored bf16 itself and nothing is launched.
static void launch_reduce_slabs_bf16(const void* ws, void* out, int ksplit,
                                     long len, void* stream) {
  if (ksplit <= 1) return;
  hipLaunchKernelGGL(reduce_slabs_bf16_kernel, reduce_slabs_grid(len),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const float*)ws, (bf16_t*)out, ksplit, len);
}

// bwd-weight always goes through slabs (nslices may be 1)
static void launch_reduce_slabs_f32(const void* ws, void* out, int nslices,
                                    long len, int accum, void* stream) {
  hipLaunchKernelGGL(reduce_slabs_f32_kernel, reduce_slabs_grid(len),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const float*)ws, (float*)out, nslices, len, accum);
}

// ------------------------------------------------------- kernel dispatch
typedef void (*FwdV1Kernel)(const bf16_t*, const bf16_t*, bf16_t*, float*,
                            ConvGeom, int, int, int, int);
// [tile: 0 = BK32 x BM128, 1 = BK64 x BM128, 2 = BK32 x BM256][FAST]
static const FwdV1Kernel kFwdV1[3][2] = {
    {conv2d_fwd_kernel<32, 128, BN, false>,
     conv2d_fwd_kernel<32, 128, BN, true>},
    {conv2d_fwd_kernel<64, 128, BN, false>,
     conv2d_fwd_kernel<64, 128, BN, true>},
    {conv2d_fwd_kernel<32, 256, BN, false>,
     conv2d_fwd_kernel<32, 256, BN, true>}};

typedef void (*BwdDataKernel)(const bf16_t*, const bf16_t*, bf16_t*, float*,
                              ConvGeom, int, int, int, int, const bf16_t*,
                              const bf16_t*, const float*, const float*,
                              float*, int);
// [BKT == 64][FAST][BNP]
static const BwdDataKernel kBwdData[2][2][2] = {
    {{conv2d_bwd_data_kernel<32, false, false>,
      conv2d_bwd_data_kernel<32, false, true>},
     {conv2d_bwd_data_kernel<32, true, false>,
      conv2d_bwd_data_kernel<32, true, true>}},
    {{conv2d_bwd_data_kernel<64, false, false>,
      conv2d_bwd_data_kernel<64, false, true>},
     {conv2d_bwd_data_kernel<64, true, false>,
      conv2d_bwd_data_kernel<64, true, true>}}};

extern "C" {

// 64 KiB zeroed device page: OOB gather lanes of the all-glds v2 kernels
// point here. Allocated lazily OUTSIDE graph capture (the engine always
// runs an eager warmup step before capturing).
static void* zpage_ptr() {
  static void* p = nullptr;
  if (p == nullptr) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(nullptr, &st);
    if (st != hipStreamCaptureStatusNone) return nullptr;  // caller falls back
    void* q = nullptr;
    if (hipMalloc(&q, 65536) != hipSuccess) return nullptr;
    (void)hipMemset(q, 0, 65536);
    p = q;
  }
  return p;
}

// ------------------------------------------------------------ route codes
// Small integers shared with cilfw/_hip_ops.py (which maps them to names) so
// a test can assert which kernel a geometry selects. Each launcher below
// branches on the SAME function that answers the query, so the two cannot
// drift apart when a threshold is retuned.
enum { FWD_V1_BK32 = 0, FWD_V1_BK64 = 1, FWD_V2_BN64 = 2, FWD_V2_BN128 = 3 };
enum { BWDD_S2_FUSED = 0, BWDD_V2 = 1, BWDD_V1_BK32 = 2, BWDD_V1_BK64 = 3 };
enum { BWDW_V2 = 0, BWDW_V1_FAST = 1, BWDW_V1_GENERIC = 2 };

// BM=256 doubles MFMA-per-barrier when M is large enough to keep the grid
// full (env-gated experiment; it runs the v1 BKT=32 kernel)
static int fwd_bm(int M) { return (M >= fwd_bm256_min_m()) ? 256 : BM; }

static int fwd_v2_eligible(int C) { return C % 8 == 0 && conv_v2_enabled(); }

// have_zp: the zero page exists (always, outside graph capture)
static int fwd_route(int M, int C, int K, int R, int S, int ksplit,
                     int have_zp) {
  int CRS = C * R * S;
  int bm = fwd_bm(M);
  if (have_zp && fwd_v2_eligible(C) && bm == BM) {
    // all-glds 2-phase kernel (v2): BK=64, tr_b16 B operand
    int shape_ok = (R == 1 && S == 1) || M >= v2_bn128_min3x3();
    if (v2_bn128_enabled() && K % 128 == 0 && shape_ok &&
        cdiv(M, BM) * cdiv(K, 128) * ksplit >= 256)
      return FWD_V2_BN128;
    return FWD_V2_BN64;
  }
  // BKT=64 only when the grid is too small for BKT=32's 2x occupancy
  // (a BN=128 v1 tile variant was tried and measured slower AND failed
  //  numerics — removed; the template's NRC generalization remains at the
  //  validated 2)
  int use64 = bm == BM && (CRS >= bk64_min_crs()) &&
              (cdiv(M, BM) * cdiv(K, BN) * ksplit < bk64_max_blocks());
  return use64 ? FWD_V1_BK64 : FWD_V1_BK32;
}

// which forward kernel cilfw_conv2d_fwd launches for this geometry
int cilfw_conv2d_fwd_route(int N, int C, int K, int R, int S, int Ho, int Wo,
                           int ksplit) {
  return fwd_route(N * Ho * Wo, C, K, R, S, ksplit, 1);
}

// rows of the (gy, 2, K) BN-statistics partials the v2 forward epilogue
// writes: one per M block
int cilfw_conv2d_fwd_bn_gy(int N, int Ho, int Wo) {
  return cdiv(N * Ho * Wo, BM);
}

void cilfw_conv2d_fwd(const void* x, const void* w, void* y, void* ws,
                      int N, int H, int W, int C, int K, int R, int S,
                      int stride, int pad, int Ho, int Wo, int ksplit,
                      void* bn_parts, void* stream) {
  ConvGeom g{N, H, W, C, K, R, S, stride, pad, pad, Ho, Wo,
             0, 0, magic40(C), magic40(S)};
  int M = N * Ho * Wo;
  int CRS = C * R * S;
  void* zp = fwd_v2_eligible(C) ? zpage_ptr() : nullptr;
  int route = fwd_route(M, C, K, R, S, ksplit, zp != nullptr);
  if (route == FWD_V2_BN128 || route == FWD_V2_BN64) {
    int bn128 = route == FWD_V2_BN128;
    dim3 grid(cdiv(M, BM), cdiv(K, bn128 ? 128 : BN), ksplit);
    hipLaunchKernelGGL(
        bn128 ? conv2d_fwd_v2_kernel<128> : conv2d_fwd_v2_kernel<BN>, grid,
        dim3(NTHREADS), 0, (hipStream_t)stream, (const bf16_t*)x,
        (const bf16_t*)w, (bf16_t*)y, (float*)ws, (const bf16_t*)zp, g, M,
        CRS, cdiv(CRS, V2BK), ksplit,
        (float*)(ksplit > 1 ? nullptr : bn_parts));
  } else {
    int bm = fwd_bm(M);
    int tile = route == FWD_V1_BK64 ? 1 : (bm == 256 ? 2 : 0);
    dim3 grid(cdiv(M, bm), cdiv(K, BN), ksplit);
    hipLaunchKernelGGL(kFwdV1[tile][C % 16 == 0], grid, dim3(NTHREADS), 0,
                       (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)w, (bf16_t*)y, (float*)ws, g, M, CRS,
                       cdiv(CRS, tile == 1 ? 64 : 32), ksplit);
  }
  launch_reduce_slabs_bf16(ws, y, ksplit, (long)M * K, stream);
}

int cilfw_conv2d_fwd_ksplit(int N, int C, int K, int R, int S, int Ho,
                            int Wo) {
  return pick_ksplit(cdiv(N * Ho * Wo, BM) * cdiv(K, BN),
                     cdiv(C * R * S, 32));
}

// ops/functional.py asks this instead of reading the knob a second time
int cilfw_bnbwd_fuse_enabled() { return bnbwd_fuse_enabled() != 0; }

static int bwd_data_v2_eligible(int M, int K, int stride) {
  return K % 8 == 0 && stride <= 2 && conv_v2_enabled() &&
         M >= conv_v2_bwd_minm();
}

// have_zp: the zero page exists (always, outside graph capture)
static int bwd_data_route(int N, int H, int W, int C, int K, int R, int S,
                          int stride, int ksplit, int have_zp) {
  int H2max = (H + 1) >> 1, W2max = (W + 1) >> 1;
  int Mc = N * H2max * W2max;
  // fused 4-class parity decomposition: grid.z = (hi%2, wi%2) class;
  // small per-class grids fall back to the single zero-structured kernel
  // (its ksplit fills the chip better there — measured)
  if (stride == 2 && (R > 1 || S > 1) && K % 16 == 0 &&
      cdiv(Mc, BM) * cdiv(C, BN) >= 128 && s2_fused_enabled())
    return BWDD_S2_FUSED;
  int M = N * H * W;
  if (have_zp && bwd_data_v2_eligible(M, K, stride)) return BWDD_V2;
  int use64 = (R * S * K >= bk64_min_crs()) &&
              (cdiv(M, BM) * cdiv(C, BN) * ksplit < bk64_max_blocks());
  return use64 ? BWDD_V1_BK64 : BWDD_V1_BK32;
}

// which bwd-data kernel cilfw_conv2d_bwd_data launches for this geometry
int cilfw_conv2d_bwd_data_route(int N, int H, int W, int C, int K, int R,
                                int S, int stride, int ksplit) {
  return bwd_data_route(N, H, W, C, K, R, S, stride, ksplit, 1);
}

int cilfw_conv2d_bwd_data_ksplit(int N, int H, int W, int C, int K, int R,
                                 int S) {
  return pick_ksplit(cdiv(N * H * W, BM) * cdiv(C, BN), cdiv(R * S * K, 32));
}

// exact predicate for "bwd-data will take the v1 ksplit==1 path and can emit
// BN-backward partials" — Python checks this before allocating the parts
// buffer; the launcher re-checks and reports what it actually did
int cilfw_conv2d_bwd_data_can_fuse_bn(int N, int H, int W, int C, int K,
                                      int R, int S, int stride) {
  if (!bnbwd_fuse_enabled() || stride != 1) return 0;
  int ks = cilfw_conv2d_bwd_data_ksplit(N, H, W, C, K, R, S);
  // v2 all-glds kernel has no BN epilogue (yet)
  int route = bwd_data_route(N, H, W, C, K, R, S, stride, ks, 1);
  return (route == BWDD_V1_BK32 || route == BWDD_V1_BK64) && ks == 1;
}

int cilfw_conv2d_bwd_data_bn_gy(int N, int H, int W) {
  return cdiv(N * H * W, BM);
}

// returns 1 when the BN-backward partials were written to bn_parts
int cilfw_conv2d_bwd_data(const void* dy, const void* w, void* dx, void* ws,
                          int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int Ho, int Wo, int ksplit,
                          const void* bn_y, const void* bn_x,
                          const void* bn_mean, const void* bn_invstd,
                          void* bn_parts, int bn_relu, void* stream) {
  ConvGeom g{N, H, W, C, K, R, S, stride, pad, pad, Ho, Wo,
             0, 0, magic40(K), magic40(S)};
  int M = N * H * W;
  int RSK = R * S * K;
  // the zero page is only needed (and only allocated) for v2 candidates
  void* zp = bwd_data_v2_eligible(M, K, stride) ? zpage_ptr() : nullptr;
  int route = bwd_data_route(N, H, W, C, K, R, S, stride, ksplit,
                             zp != nullptr);
  if (route == BWDD_S2_FUSED) {
    int Mc = N * ((H + 1) >> 1) * ((W + 1) >> 1);
    dim3 grid(cdiv(Mc, BM), cdiv(C, BN), 4);
    hipLaunchKernelGGL((conv2d_bwd_data_s2_kernel<32>), grid, dim3(NTHREADS),
                       0, (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)w, (bf16_t*)dx, g);
    return 0;
  }
  dim3 grid(cdiv(M, BM), cdiv(C, BN), ksplit);
  int bnp = 0;
  if (route == BWDD_V2) {  // all-glds 2-phase kernel (v2)
    hipLaunchKernelGGL(conv2d_bwd_data_v2_kernel, grid, dim3(NTHREADS), 0,
                       (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)w, (bf16_t*)dx, (float*)ws,
                       (const bf16_t*)zp, g, M, RSK, cdiv(RSK, V2BK), ksplit);
  } else {
    int bk64 = route == BWDD_V1_BK64;
    int fast = (K % 16 == 0) && stride <= 2;  // FAST path shift-divides
    // BN-backward partial-sum epilogue: only the ksplit==1 v1 path
    // materializes final dx inside the MFMA kernel (split-K writes fp32
    // slabs instead)
    bnp = bn_parts != nullptr && ksplit == 1 && stride == 1 &&
          bnbwd_fuse_enabled();
    hipLaunchKernelGGL(kBwdData[bk64][fast][bnp], grid, dim3(NTHREADS), 0,
                       (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)w, (bf16_t*)dx, (float*)ws, g, M, RSK,
                       cdiv(RSK, bk64 ? 64 : 32), ksplit,
                       (const bf16_t*)bn_y, (const bf16_t*)bn_x,
                       (const float*)bn_mean, (const float*)bn_invstd,
                       (float*)bn_parts, bn_relu);
  }
  launch_reduce_slabs_bf16(ws, dx, ksplit, (long)M * C, stream);
  return bnp;
}

static int bwd_weight_v2_eligible(int C, int K, int accum) {
  return C % 8 == 0 && K % 8 == 0 && accum == 0 && conv_v2_enabled();
}

// have_zp: the zero page exists (always, outside graph capture)
static int bwd_weight_route(int C, int K, int accum, int have_zp) {
  if (have_zp && bwd_weight_v2_eligible(C, K, accum)) return BWDW_V2;
  return (C % 8 == 0) ? BWDW_V1_FAST : BWDW_V1_GENERIC;
}

// which bwd-weight kernel cilfw_conv2d_bwd_weight launches; the spatial
// geometry is part of the signature so a later M-dependent threshold does
// not change the ABI (today only C, K and accum decide)
int cilfw_conv2d_bwd_weight_route(int N, int C, int K, int R, int S, int Ho,
                                  int Wo, int accum) {
  (void)N; (void)R; (void)S; (void)Ho; (void)Wo;
  return bwd_weight_route(C, K, accum, 1);
}

void cilfw_conv2d_bwd_weight(const void* dy, const void* x, void* dw,
                             void* ws, int N, int H, int W, int C, int K,
                             int R, int S, int stride, int pad, int Ho,
                             int Wo, int nslices, int accum, void* stream) {
  ConvGeom g{N, H, W, C, K, R, S, stride, pad, pad, Ho, Wo,
             magic40(Ho * Wo), magic40(Wo), magic40(C), magic40(S)};
  int M = N * Ho * Wo;
  if (M >= (1 << 22) || Ho * Wo >= (1 << 14)) {
    fprintf(stderr, "cilfw_conv2d_bwd_weight: magic-division range exceeded "
            "(M=%d HoWo=%d)\n", M, Ho * Wo);
    abort();
  }
  int CRS = C * R * S;
  int slice_len = cdiv(cdiv(M, nslices), WBK) * WBK;
  dim3 grid(cdiv(CRS, WBM), cdiv(K, BN), nslices);
  void* zp = bwd_weight_v2_eligible(C, K, accum) ? zpage_ptr() : nullptr;
  int route = bwd_weight_route(C, K, accum, zp != nullptr);
  if (route == BWDW_V2)  // all-glds 2-phase kernel (v2)
    hipLaunchKernelGGL(conv2d_bwd_weight_v2_kernel, grid, dim3(NTHREADS), 0,
                       (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)x, (float*)ws, (const bf16_t*)zp, g,
                       M, CRS, slice_len);
  else
    hipLaunchKernelGGL(route == BWDW_V1_FAST
                           ? conv2d_bwd_weight_kernel<true>
                           : conv2d_bwd_weight_kernel<false>,
                       grid, dim3(NTHREADS), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (const bf16_t*)x, (float*)ws, g, M,
                       CRS, slice_len);
  launch_reduce_slabs_f32(ws, dw, nslices, (long)CRS * K, accum, stream);
}

void cilfw_im2col_smallc(const void* x, const void* mt, void* col,
                         int N, int H, int W, int C, int R, int S,
                         int stride, int pad, int Ho, int Wo, int CRSpad,
                         void* stream) {
  ConvGeom g{N, H, W, C, 0, R, S, stride, pad, pad, Ho, Wo};
  int M = N * Ho * Wo;
  long total = (long)M * R * S;
  hipLaunchKernelGGL(im2col_smallc_kernel,
                     dim3((int)cdiv((long)total, (long)NTHREADS)),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (const int*)mt, (bf16_t*)col, g, M,
                     CRSpad, total);
}

void cilfw_fill_mtable(void* mt, int M, int HoWo, int Wo, int stride,
                       void* stream) {
  hipLaunchKernelGGL(fill_mtable_kernel, dim3(cdiv(M, NTHREADS)),
                     dim3(NTHREADS), 0, (hipStream_t)stream, (int*)mt, M,
                     HoWo, Wo, stride);
}

int cilfw_conv2d_bwd_weight_nslices(int N, int C, int K, int R, int S,
                                    int Ho, int Wo) {
  int M = N * Ho * Wo;
  int CRS = C * R * S;
  int nblocks = cdiv(CRS, WBM) * cdiv(K, BN);
  int ns = cdiv(dw_target(), max(nblocks, 1));
  int max_ns = max(cdiv(M, WBK * 8), 1);  // keep >= 8 K-steps per slice
  if (ns > max_ns) ns = max_ns;
  if (ns < 1) ns = 1;
  if (ns > 64) ns = 64;
  return ns;
}

}  // extern "C"
