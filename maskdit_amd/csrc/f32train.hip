// fp32 TRAINING of the unmasked stage (the reference's "finetune with unmasking", README.md:102-119: mask_ratio 0,
// `train.py --no_amp`): what the exact-fp32 forward of f32path.hip lacks for a backward pass.
//
//   mdt_gemm_f32_tn          C[z] (+)= A[z]^T B[z]: the weight gradient of every nn.Linear (reduction over the tokens, both
//                            operands token-major) and, batched over (sample, head), dK = dS^T Q and dV = P^T dO
//   mdt_colsum_f32           bias gradients
//   mdt_attn_f32_bwd         backward of timm Attention on the packed fp32 qkv buffer, composed of batched mdt_gemm_f32 /
//                            mdt_gemm_f32_tn launches, mdt_softmax_rows_f32 and one row kernel (dS from P and dP)
//   mdt_ln_modulate_bwd_f32  LayerNorm + modulate backward: dx, per-sample dshift / dscale
//   mdt_gate_bwd_f32         backward of `x + gate * f`: df, per-sample dgate
//   mdt_gate_res_f32, mdt_gelu_f32, mdt_gelu_bwd_f32, mdt_silu_bwd_f32   elementwise passes of the training forward / backward
//
// Data gradients dX = dY W need nothing new: mdt_gemm_f32 with b_kmajor = 1 reads W [N, K] as its K-major operand.
// Everything here is DETERMINISTIC: no atomics; every reduction that is split (over token chunks, over row lanes) writes
// its partial sums and folds them in index order, so two runs give identical bits.
//
// GEMM design.  The fp32-input matrix instruction (v_mfma_f32_32x32x2_f32, as mdt_gemm_f32) bounds the kernel: per 32-token
// K-tile a wave issues 16 MB NB MFMAs of 64 clocks against 16 (MB + NB) 4-byte LDS reads, so the plain structure of
// f32path.hip's register-staged form is kept: (32 WM MB) x (32 WN NB) output tile, 4 waves, K-tiles of 32 tokens staged
// through registers into a double-buffered LDS image [token][column] (the operands' own layout: rows are stored as they
// are loaded, a fragment read takes 32 consecutive floats of one token row -- conflict-free), one workgroup barrier per
// K-tile, waits placed by hipcc.  The token dimension is split into fixed chunks (mdt_gemm_f32_tn_ws_floats explains the
// rule); with more than one chunk every chunk's tile goes to the workspace and tn_fold_kernel adds them in chunk order.
#include "common.h"
#include "../../include/maskdit_hip.h"
#include <math.h>

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace f32t {

struct TnParams {
  const float* A; long lda;
  const float* B; long ldb;
  int M, N1, N2;
  float* C; long ldc;
  int accumulate;
  int heads;
  long a_sb, a_sh, b_sb, b_sh, c_sb, c_sh;
  int chunk, nsplit;
  float* ws;
  int vec_ok;  // 16-byte stores to C are legal
};

// exact-form activations (restated from f32path.hip: torch's F.gelu(approximate='tanh') / F.silu in fp32)
__device__ __forceinline__ float gelu_tanh_f32(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return 0.5f * x * (1.f + tanhf(u));
}
__device__ __forceinline__ float gelu_tanh_grad_f32(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  const float t = tanhf(u);
  const float du = 0.7978845608028654f * (1.f + 3.f * 0.044715f * x * x);
  return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * du;
}
__device__ __forceinline__ float silu_grad_f32(float x) {
  const float s = 1.f / (1.f + expf(-x));
  return s * (1.f + x * (1.f - s));
}

// grid (tiles1 * tiles2, nsplit, batch)
template <int WM, int WN, int MB, int NB>
__global__ __launch_bounds__(256, 2) void gemm_f32_tn_kernel(const TnParams p, const int tiles2) {
  constexpr int BKT = 32, BM = WM * MB * 32, BN = WN * NB * 32;
  constexpr int A_CPR = BM / 4, B_CPR = BN / 4;                    // 16-byte chunks per token row
  constexpr int A_CH = BKT * A_CPR / 256, B_CH = BKT * B_CPR / 256;  // chunks per thread and K-tile
  static_assert(WM * WN == 4, "four waves");
  static_assert(A_CH >= 1 && B_CH >= 1, "tile too small for 256 threads");
  __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * BKT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int t1 = blockIdx.x / tiles2, t2 = blockIdx.x - t1 * tiles2;
  const int n1_0 = t1 * BM, n2_0 = t2 * BN;
  const int s = blockIdx.y, z = blockIdx.z, zb = z / p.heads, zh = z - zb * p.heads;
  const int ms = s * p.chunk, me = min(ms + p.chunk, p.M);
  const float* __restrict__ A = p.A + zb * p.a_sb + zh * p.a_sh;
  const float* __restrict__ Bm = p.B + zb * p.b_sb + zh * p.b_sh;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // global -> registers one K-tile ahead; rows at or beyond the chunk's end and columns at or beyond N1 / N2 read as zeros
  // (their addresses are clamped into the operand)
  f32x4 ga[A_CH], gb[B_CH];
  const float* pa[A_CH];
  const float* pb[B_CH];
  bool oka[A_CH], okb[B_CH];
  int kra[A_CH], krb[B_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int q = tid + 256 * i, c = q % A_CPR;
    kra[i] = q / A_CPR;
    oka[i] = (n1_0 + 4 * c) < p.N1;
    pa[i] = A + min(n1_0 + 4 * c, p.N1 - 4);
  }
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    const int q = tid + 256 * i, c = q % B_CPR;
    krb[i] = q / B_CPR;
    okb[i] = (n2_0 + 4 * c) < p.N2;
    pb[i] = Bm + min(n2_0 + 4 * c, p.N2 - 4);
  }
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = ms + k0 + kra[i];
      const f32x4 v = *(const f32x4*)(pa[i] + (long)min(row, p.M - 1) * p.lda);
      ga[i] = (oka[i] && row < me) ? v : zero4;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int row = ms + k0 + krb[i];
      const f32x4 v = *(const f32x4*)(pb[i] + (long)min(row, p.M - 1) * p.ldb);
      gb[i] = (okb[i] && row < me) ? v : zero4;
    }
  };
  auto lstore = [&](int buf) {
    float* la = lds[buf];
    float* lb = lds[buf] + BM * BKT;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) *(f32x4*)(la + 4 * (tid + 256 * i)) = ga[i];  // [token][BM]
#pragma unroll
    for (int i = 0; i < B_CH; ++i) *(f32x4*)(lb + 4 * (tid + 256 * i)) = gb[i];  // [token][BN]
  };
  const int r = lane & 31, kh = lane >> 5;
  // lane (r, kh) feeds token k = 8 j + 4 kh + e of a K-tile to MFMA e of step group j -- the same permutation for A and B, so
  // the sum runs over all 32 tokens.  B first: the accumulator block is the transposed output block (see f32path.hip), a
  // lane holds output row n1 = its A column and four consecutive n2 per register quad.
  auto compute = [&](int buf) {
    const float* la = lds[buf] + wm * MB * 32 + r;
    const float* lb = lds[buf] + BM * BKT + wn * NB * 32 + r;
#pragma unroll
    for (int j = 0; j < BKT / 8; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 8 * j + 4 * kh + e;
        float fa[MB], fb[NB];
#pragma unroll
        for (int i = 0; i < MB; ++i) fa[i] = la[k * BM + 32 * i];
#pragma unroll
        for (int i = 0; i < NB; ++i) fb[i] = lb[k * BN + 32 * i];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int jj = 0; jj < NB; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[jj], fa[i], acc[i][jj], 0, 0, 0);
      }
    }
  };
  const int nk = (me - ms + BKT - 1) / BKT;
  gload(0);
  lstore(0);
  __syncthreads();
  // tile kt + 1 is stored into the buffer tile kt - 1 was read from; every wave finished those reads before the barrier
  // that ended iteration kt - 1
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) gload((kt + 1) * BKT);
    compute(buf);
    if (more) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: one chunk -> C itself (+= when accumulate), several -> this chunk's slab of the workspace [z][s][N1][N2]
  const bool direct = p.nsplit == 1;
  float* __restrict__ out = direct ? p.C + zb * p.c_sb + zh * p.c_sh : p.ws + ((long)z * p.nsplit + s) * p.N1 * (long)p.N2;
  const long ld = direct ? p.ldc : (long)p.N2;
  const bool vec = direct ? p.vec_ok != 0 : true;  // (N2 % 4 == 0 and the workspace is 16-byte aligned)
  const bool accum = direct && p.accumulate;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int n1 = n1_0 + (wm * MB + i) * 32 + r;
    if (n1 >= p.N1) continue;
    float* orow = out + (long)n1 * ld;
#pragma unroll
    for (int jj = 0; jj < NB; ++jj) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int nq = n2_0 + (wn * NB + jj) * 32 + 8 * q4 + 4 * kh;
        if (nq >= p.N2) continue;  // N2 % 4 == 0: a quad is inside or outside as a whole
        f32x4 y = (f32x4){acc[i][jj][4 * q4], acc[i][jj][4 * q4 + 1], acc[i][jj][4 * q4 + 2], acc[i][jj][4 * q4 + 3]};
        if (vec) {
          if (accum) {
            const f32x4 c0 = *(const f32x4*)(orow + nq);
            y = (f32x4){c0[0] + y[0], c0[1] + y[1], c0[2] + y[2], c0[3] + y[3]};
          }
          *(f32x4*)(orow + nq) = y;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) orow[nq + e] = accum ? orow[nq + e] + y[e] : y[e];
        }
      }
    }
  }
}

// C[z][n1, n2 .. n2 + 3] (+)= sum over the chunks in index order
__global__ __launch_bounds__(256) void tn_fold_kernel(const TnParams p, const long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nq = p.N2 >> 2;
  const long row = idx / nq;  // z * N1 + n1
  const int q = (int)(idx - row * nq);
  const int z = (int)(row / p.N1), n1 = (int)(row - (long)z * p.N1);
  const int zb = z / p.heads, zh = z - zb * p.heads;
  const long slab = (long)p.N1 * p.N2;
  const float* src = p.ws + (long)z * p.nsplit * slab + (long)n1 * p.N2 + 4 * q;
  float* dst = p.C + zb * p.c_sb + zh * p.c_sh + (long)n1 * p.ldc + 4 * q;
  f32x4 sum = *(const f32x4*)src;
  for (int s = 1; s < p.nsplit; ++s) {
    const f32x4 v = *(const f32x4*)(src + s * slab);
    sum = (f32x4){sum[0] + v[0], sum[1] + v[1], sum[2] + v[2], sum[3] + v[3]};
  }
  if (p.vec_ok) {
    if (p.accumulate) {
      const f32x4 c0 = *(const f32x4*)dst;
      sum = (f32x4){c0[0] + sum[0], c0[1] + sum[1], c0[2] + sum[2], c0[3] + sum[3]};
    }
    *(f32x4*)dst = sum;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = p.accumulate ? dst[e] + sum[e] : sum[e];
  }
}

template <int WM, int WN, int MB, int NB>
int launch_tn(const TnParams& p, int batch, hipStream_t stream) {
  constexpr int BM = WM * MB * 32, BN = WN * NB * 32;
  const int tiles1 = cdiv(p.N1, BM), tiles2 = cdiv(p.N2, BN);
  hipLaunchKernelGGL((gemm_f32_tn_kernel<WM, WN, MB, NB>), dim3(tiles1 * tiles2, p.nsplit, batch), dim3(256), 0, stream, p, tiles2);
  return mdt_check_launch("gemm_f32_tn");
}

// ---- ordered column reductions ----------------------------------------------------------------------------------------
// A workgroup of 256 threads covers 64 columns (16 quads) x 16 row lanes: row lane rl adds rows rl, rl + 16, ... of its
// range in that order, the 16 partial sums meet in LDS and are added in row-lane order.  Nothing depends on timing.
#define RL 16
__device__ __forceinline__ f32x4 fold16(f32x4 v, float (*red)[68], int cq, int rl) {
  *(f32x4*)(&red[rl][4 * cq]) = v;
  __syncthreads();
  f32x4 s = *(const f32x4*)(&red[0][4 * cq]);
  for (int k = 1; k < RL; ++k) {
    const f32x4 u = *(const f32x4*)(&red[k][4 * cq]);
    s = (f32x4){s[0] + u[0], s[1] + u[1], s[2] + u[2], s[3] + u[3]};
  }
  __syncthreads();
  return s;  // (every row lane holds the same sum; row lane 0 stores it)
}

// grid (cdiv(N, 64), nchunks): dst[chunk][n] = sum of rows [chunk * rows_per_chunk, ...) of in[:, n]
__global__ __launch_bounds__(256) void colsum_f32_kernel(const float* __restrict__ in, long ld, float* __restrict__ dst, long dst_ld,
                                                         int M, int N, int rows_per_chunk, int accumulate) {
  __shared__ __attribute__((aligned(16))) float red[RL][68];
  const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;
  const bool ok = col < N;
  const int m0 = blockIdx.y * rows_per_chunk, m1 = min(m0 + rows_per_chunk, M);
  f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (ok)
    for (int m = m0 + rl; m < m1; m += RL) {
      const f32x4 v = *(const f32x4*)(in + (long)m * ld + col);
      s = (f32x4){s[0] + v[0], s[1] + v[1], s[2] + v[2], s[3] + v[3]};
    }
  s = fold16(s, red, cq, rl);
  if (ok && rl == 0) {
    float* o = dst + (long)blockIdx.y * dst_ld + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = accumulate ? o[e] + s[e] : s[e];
  }
}

// out[n] (+)= sum over the chunk partials in index order
__global__ __launch_bounds__(256) void colsum_fold_kernel(const float* __restrict__ part, float* __restrict__ out, int N, int nchunks,
                                                          int accumulate) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = part[n];
  for (int c = 1; c < nchunks; ++c) s += part[(long)c * N + n];
  out[n] = accumulate ? out[n] + s : s;
}

// ---- LayerNorm + modulate backward ---------------------------------------------------------------------------------------
// xn = xhat (1 + scale[b]) + shift[b], xhat = (x - mean) rstd (models/maskdit.py:19-20,177; eps 1e-6):
//   g = dxn (1 + scale);  dx (+)= rstd (g - mean(g) - xhat mean(g xhat));  one wave per row, statistics recomputed as
// mdt_ln_modulate_f32 computes them and left in stats[2 row] = (mean, rstd) for the per-sample reduction below.
template <int NVT>
__global__ __launch_bounds__(256) void ln_modulate_bwd_f32_kernel(const float* __restrict__ dxn, const float* __restrict__ x,
                                                                  const float* __restrict__ scale, int mod_ld, int rows_per_sample,
                                                                  float* __restrict__ dx, int accumulate, float* __restrict__ stats,
                                                                  int M, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nv = D >> 2;
  const float* xr = x + (long)row * D;
  const float* gr = dxn + (long)row * D;
  const float* sc = scale + (long)(row / rows_per_sample) * mod_ld;
  f32x4 v[NVT], g[NVT];
  int col[NVT];
  float own[NVT];
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    const int c = lane + 64 * i;
    own[i] = c < nv ? 1.f : 0.f;
    col[i] = 4 * min(c, nv - 1);
    v[i] = *(const f32x4*)(xr + col[i]);
    const f32x4 d = *(const f32x4*)(gr + col[i]);
    const f32x4 m = *(const f32x4*)(sc + col[i]);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[i][e] = d[e] * (1.f + m[e]);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NVT; ++i) s += own[i] * (v[i][0] + v[i][1] + v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    float qi = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[i][e] - mean;
      qi += d * d;
    }
    q += own[i] * qi;
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + 1e-6f);
  float c1 = 0.f, c2 = 0.f;
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[i][e] = (v[i][e] - mean) * rstd;  // xhat
      a1 += g[i][e];
      a2 += g[i][e] * v[i][e];
    }
    c1 += own[i] * a1;
    c2 += own[i] * a2;
  }
  c1 = wave_sum(c1) / (float)D;
  c2 = wave_sum(c2) / (float)D;
  float* o = dx + (long)row * D;
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    if (own[i] == 0.f) continue;
    f32x4 rr;
#pragma unroll
    for (int e = 0; e < 4; ++e) rr[e] = rstd * (g[i][e] - c1 - v[i][e] * c2);
    if (accumulate) {
      const f32x4 o0 = *(const f32x4*)(o + col[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) rr[e] += o0[e];
    }
    *(f32x4*)(o + col[i]) = rr;
  }
  if (lane == 0) {
    stats[2 * (long)row] = mean;
    stats[2 * (long)row + 1] = rstd;
  }
}

// grid (cdiv(D, 64), samples): dshift[b, d] = sum_l dxn[l, d], dscale[b, d] = sum_l dxn[l, d] xhat[l, d] over the sample's rows
__global__ __launch_bounds__(256) void ln_mod_reduce_f32_kernel(const float* __restrict__ dxn, const float* __restrict__ x,
                                                                const float* __restrict__ stats, int rows_per_sample,
                                                                float* __restrict__ dshift, float* __restrict__ dscale, int dmod_ld,
                                                                int M, int D) {
  __shared__ __attribute__((aligned(16))) float red[RL][68];
  const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;
  const bool ok = col < D;
  const long r0 = (long)blockIdx.y * rows_per_sample;
  const long r1 = min(r0 + rows_per_sample, (long)M);
  f32x4 ssh = (f32x4){0.f, 0.f, 0.f, 0.f}, ssc = ssh;
  if (ok)
    for (long row = r0 + rl; row < r1; row += RL) {
      const f32x4 d = *(const f32x4*)(dxn + row * D + col);
      const f32x4 v = *(const f32x4*)(x + row * D + col);
      const float mean = stats[2 * row], rstd = stats[2 * row + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ssh[e] += d[e];
        ssc[e] += d[e] * ((v[e] - mean) * rstd);
      }
    }
  ssh = fold16(ssh, red, cq, rl);
  ssc = fold16(ssc, red, cq, rl);
  if (ok && rl == 0) {
    float* o1 = dshift + (long)blockIdx.y * dmod_ld + col;
    float* o2 = dscale + (long)blockIdx.y * dmod_ld + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o1[e] = ssh[e];
      o2[e] = ssc[e];
    }
  }
}

// grid (cdiv(D, 64), samples): df = gate[b] dy, dgate[b, d] = sum_l dy[l, d] f[l, d]   (`x + gate * f`, models/maskdit.py:190-191)
__global__ __launch_bounds__(256) void gate_bwd_f32_kernel(const float* __restrict__ dy, const float* __restrict__ f,
                                                           const float* __restrict__ gate, int gate_ld, int rows_per_sample,
                                                           float* __restrict__ df, float* __restrict__ dgate, int dgate_ld, int M, int D) {
  __shared__ __attribute__((aligned(16))) float red[RL][68];
  const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;
  const bool ok = col < D;
  const long r0 = (long)blockIdx.y * rows_per_sample;
  const long r1 = min(r0 + rows_per_sample, (long)M);
  f32x4 sg = (f32x4){0.f, 0.f, 0.f, 0.f}, g4 = sg;
  if (ok) {
    const float* gp = gate + (long)blockIdx.y * gate_ld + col;
    g4 = (f32x4){gp[0], gp[1], gp[2], gp[3]};
    for (long row = r0 + rl; row < r1; row += RL) {
      const f32x4 d = *(const f32x4*)(dy + row * D + col);
      const f32x4 v = *(const f32x4*)(f + row * D + col);
      *(f32x4*)(df + row * D + col) = (f32x4){g4[0] * d[0], g4[1] * d[1], g4[2] * d[2], g4[3] * d[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) sg[e] += d[e] * v[e];
    }
  }
  sg = fold16(sg, red, cq, rl);
  if (ok && rl == 0) {
    float* o = dgate + (long)blockIdx.y * dgate_ld + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = sg[e];
  }
}

// out[row, :] = res[row, :] + gate[row / rows_per_sample, :] * f[row, :]; 4 floats per thread
__global__ __launch_bounds__(256) void gate_res_f32_kernel(const float* __restrict__ res, const float* __restrict__ f,
                                                           const float* __restrict__ gate, int gate_ld, int rows_per_sample,
                                                           float* __restrict__ out, long nq, int Dq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  const long row = i / Dq;
  const int cq = (int)(i - row * Dq);
  const float* gp = gate + (row / rows_per_sample) * gate_ld + 4 * cq;
  const f32x4 a = *(const f32x4*)(res + 4 * i);
  const f32x4 b = *(const f32x4*)(f + 4 * i);
  *(f32x4*)(out + 4 * i) = (f32x4){a[0] + gp[0] * b[0], a[1] + gp[1] * b[1], a[2] + gp[2] * b[2], a[3] + gp[3] * b[3]};
}

// mode 0: out = gelu_tanh(a); 1: out = a * gelu_tanh'(b); 2: out = a * silu'(b)
template <int MODE>
__global__ __launch_bounds__(256) void act_f32_kernel(const float* a, const float* b, float* out, long n) {  // (out may be a: no __restrict__)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (MODE == 0) out[i] = gelu_tanh_f32(a[i]);
  else if (MODE == 1) out[i] = a[i] * gelu_tanh_grad_f32(b[i]);
  else out[i] = a[i] * silu_grad_f32(b[i]);
}

// dS[r, :] = scale * P[r, :] o (dP[r, :] - sum_j P[r, j] dP[r, j]) in place of dP; one wave per row
__global__ __launch_bounds__(256) void attn_ds_rows_f32_kernel(const float* __restrict__ P, float* __restrict__ dP, long R, int n,
                                                               float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* pr = P + row * n;
  float* dr = dP + row * n;
  float s = 0.f;
  for (int j = lane; j < n; j += 64) s += pr[j] * dr[j];
  s = wave_sum(s);
  for (int j = lane; j < n; j += 64) dr[j] = scale * pr[j] * (dr[j] - s);
}

}  // namespace f32t

// ---- host entries ------------------------------------------------------------------------------------------------------

// The token dimension is cut into chunks of `chunk` rows (a multiple of the 32-row K-tile): as many chunks as it takes to
// give the device ~1024 workgroups, never shorter than 256 rows.  A function of the shape alone, so the summation order --
// and with it every bit of the result -- is fixed per shape.
static void tn_split(int M, int N1, int N2, int batch, int* chunk, int* nsplit) {
  const int bn = N2 > 64 ? 128 : (N2 > 32 ? 64 : 32);
  const long tiles = (long)cdiv(N1, 128) * cdiv(N2, bn) * batch;
  long want = (1024 + tiles - 1) / tiles;
  const long most = cdiv(M, 256);
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int ch = cdiv(cdiv(M, want), 32) * 32;
  *chunk = ch;
  *nsplit = cdiv(M, ch);
}

extern "C" long mdt_gemm_f32_tn_ws_floats(int M, int N1, int N2, int batch) {
  if (M <= 0 || N1 <= 0 || N2 <= 0) return 0;
  if (batch < 1) batch = 1;
  int chunk, nsplit;
  tn_split(M, N1, N2, batch, &chunk, &nsplit);
  return nsplit > 1 ? (long)nsplit * batch * N1 * N2 : 0L;
}

extern "C" int mdt_gemm_f32_tn(const mdt_gemm_f32_tn_args* a, mdt_stream_t stream) {
  MDT_REQUIRE(a && a->A && a->B && a->C, "gemm_f32_tn: null pointer");
  MDT_REQUIRE(a->M > 0 && a->N1 >= 4 && a->N2 >= 4 && a->N1 % 4 == 0 && a->N2 % 4 == 0,
              "gemm_f32_tn: M > 0, N1 and N2 positive multiples of 4");
  MDT_REQUIRE(a->lda % 4 == 0 && a->ldb % 4 == 0 && a->lda >= a->N1 && a->ldb >= a->N2 &&
              (((uintptr_t)a->A | (uintptr_t)a->B) & 15) == 0, "gemm_f32_tn: operand rows must be 16-byte aligned and hold N1 / N2 columns");
  MDT_REQUIRE(a->ldc >= a->N2, "gemm_f32_tn: ldc < N2");
  const int batch = a->batch > 0 ? a->batch : 1;
  const int heads = a->heads > 0 ? a->heads : 1;
  MDT_REQUIRE(batch % heads == 0 && batch <= 65535, "gemm_f32_tn: batch must be a multiple of heads and <= 65535");
  MDT_REQUIRE(((a->a_stride_b | a->a_stride_h | a->b_stride_b | a->b_stride_h) & 3) == 0,
              "gemm_f32_tn: batch strides must be multiples of 4 elements");
  f32t::TnParams p;
  p.A = a->A; p.lda = a->lda; p.B = a->B; p.ldb = a->ldb;
  p.M = a->M; p.N1 = a->N1; p.N2 = a->N2;
  p.C = a->C; p.ldc = a->ldc; p.accumulate = a->accumulate != 0;
  p.heads = heads;
  p.a_sb = a->a_stride_b; p.a_sh = a->a_stride_h; p.b_sb = a->b_stride_b; p.b_sh = a->b_stride_h;
  p.c_sb = a->c_stride_b; p.c_sh = a->c_stride_h;
  tn_split(a->M, a->N1, a->N2, batch, &p.chunk, &p.nsplit);
  MDT_REQUIRE(p.nsplit <= 65535, "gemm_f32_tn: too many token chunks");
  const long need = p.nsplit > 1 ? (long)p.nsplit * batch * a->N1 * a->N2 : 0L;
  MDT_REQUIRE(need == 0 || (a->ws && a->ws_floats >= need && ((uintptr_t)a->ws & 15) == 0),
              "gemm_f32_tn: workspace missing, unaligned or smaller than mdt_gemm_f32_tn_ws_floats()");
  p.ws = a->ws;
  p.vec_ok = a->ldc % 4 == 0 && ((uintptr_t)a->C & 15) == 0 && ((a->c_stride_b | a->c_stride_h) & 3) == 0;
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (a->N2 > 64) rc = f32t::launch_tn<2, 2, 2, 2>(p, batch, st);
  else if (a->N2 > 32) rc = f32t::launch_tn<4, 1, 1, 2>(p, batch, st);
  else rc = f32t::launch_tn<4, 1, 1, 1>(p, batch, st);
  if (rc != MDT_OK || p.nsplit == 1) return rc;
  const long total = (long)batch * a->N1 * (a->N2 / 4);
  MDT_REQUIRE(cdiv(total, 256) > 0, "gemm_f32_tn: output too large");
  hipLaunchKernelGGL(f32t::tn_fold_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, p, total);
  return mdt_check_launch("gemm_f32_tn (fold)");
}

#define COLSUM_ROWS 512
extern "C" long mdt_colsum_f32_ws_floats(int M, int N) {
  const int nch = cdiv(M, COLSUM_ROWS);
  return nch > 1 ? (long)nch * N : 0L;
}

extern "C" int mdt_colsum_f32(const float* in, long ld, float* out, float* ws, long ws_floats, int M, int N, int accumulate,
                              mdt_stream_t stream) {
  MDT_REQUIRE(in && out, "colsum_f32: null pointer");
  MDT_REQUIRE(M > 0 && N >= 4 && N % 4 == 0 && ld % 4 == 0 && ld >= N && ((uintptr_t)in & 15) == 0,
              "colsum_f32: M > 0, N a positive multiple of 4, 16-byte aligned rows");
  const int nch = cdiv(M, COLSUM_ROWS);
  MDT_REQUIRE(nch <= 65535, "colsum_f32: too many rows");
  MDT_REQUIRE(nch == 1 || (ws && ws_floats >= (long)nch * N), "colsum_f32: workspace missing or smaller than mdt_colsum_f32_ws_floats()");
  const hipStream_t st = (hipStream_t)stream;
  if (nch == 1) {
    hipLaunchKernelGGL(f32t::colsum_f32_kernel, dim3(cdiv(N, 64), 1), dim3(256), 0, st, in, ld, out, 0L, M, N, COLSUM_ROWS, accumulate != 0);
    return mdt_check_launch("colsum_f32");
  }
  hipLaunchKernelGGL(f32t::colsum_f32_kernel, dim3(cdiv(N, 64), nch), dim3(256), 0, st, in, ld, ws, (long)N, M, N, COLSUM_ROWS, 0);
  int rc = mdt_check_launch("colsum_f32");
  if (rc != MDT_OK) return rc;
  hipLaunchKernelGGL(f32t::colsum_fold_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, ws, out, N, nch, accumulate != 0);
  return mdt_check_launch("colsum_f32 (fold)");
}

extern "C" int mdt_ln_modulate_bwd_f32(const float* dxn, const float* x, const float* scale, int mod_ld, int rows_per_sample,
                                       float* dx, int accumulate, float* dshift, float* dscale, int dmod_ld, float* stats_ws,
                                       int M, int D, mdt_stream_t stream) {
  MDT_REQUIRE(dxn && x && scale && dx && dshift && dscale && stats_ws, "ln_modulate_bwd_f32: null pointer");
  MDT_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1280 && M > 0 && rows_per_sample > 0 && mod_ld % 4 == 0, "ln_modulate_bwd_f32: bad shape");
  MDT_REQUIRE((((uintptr_t)dxn | (uintptr_t)x | (uintptr_t)scale | (uintptr_t)dx) & 15) == 0, "ln_modulate_bwd_f32: 16-byte aligned buffers");
  const int samples = cdiv(M, rows_per_sample);
  MDT_REQUIRE(samples <= 65535, "ln_modulate_bwd_f32: more than 65535 samples");
  const dim3 grid(cdiv(M, 4)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define LNB_GO(NVT) hipLaunchKernelGGL(f32t::ln_modulate_bwd_f32_kernel<NVT>, grid, block, 0, st, dxn, x, scale, mod_ld, rows_per_sample, \
                                       dx, accumulate != 0, stats_ws, M, D)
  switch (cdiv(D / 4, 64)) {
    case 1: LNB_GO(1); break;
    case 2: LNB_GO(2); break;
    case 3: LNB_GO(3); break;
    case 4: LNB_GO(4); break;
    default: LNB_GO(5); break;
  }
#undef LNB_GO
  int rc = mdt_check_launch("ln_modulate_bwd_f32");
  if (rc != MDT_OK) return rc;
  hipLaunchKernelGGL(f32t::ln_mod_reduce_f32_kernel, dim3(cdiv(D, 64), samples), block, 0, st, dxn, x, stats_ws, rows_per_sample, dshift,
                     dscale, dmod_ld, M, D);
  return mdt_check_launch("ln_modulate_bwd_f32 (reduce)");
}

extern "C" int mdt_gate_bwd_f32(const float* dy, const float* f, const float* gate, int gate_ld, int rows_per_sample, float* df,
                                float* dgate, int dgate_ld, int M, int D, mdt_stream_t stream) {
  MDT_REQUIRE(dy && f && gate && df && dgate, "gate_bwd_f32: null pointer");
  MDT_REQUIRE(D % 4 == 0 && D >= 4 && M > 0 && rows_per_sample > 0, "gate_bwd_f32: bad shape");
  MDT_REQUIRE((((uintptr_t)dy | (uintptr_t)f | (uintptr_t)df) & 15) == 0, "gate_bwd_f32: 16-byte aligned buffers");
  const int samples = cdiv(M, rows_per_sample);
  MDT_REQUIRE(samples <= 65535, "gate_bwd_f32: more than 65535 samples");
  hipLaunchKernelGGL(f32t::gate_bwd_f32_kernel, dim3(cdiv(D, 64), samples), dim3(256), 0, (hipStream_t)stream, dy, f, gate, gate_ld,
                     rows_per_sample, df, dgate, dgate_ld, M, D);
  return mdt_check_launch("gate_bwd_f32");
}

extern "C" int mdt_gate_res_f32(const float* res, const float* f, const float* gate, int gate_ld, int rows_per_sample, float* out,
                                int M, int D, mdt_stream_t stream) {
  MDT_REQUIRE(res && f && gate && out, "gate_res_f32: null pointer");
  MDT_REQUIRE(D % 4 == 0 && D >= 4 && M > 0 && rows_per_sample > 0, "gate_res_f32: bad shape");
  MDT_REQUIRE((((uintptr_t)res | (uintptr_t)f | (uintptr_t)out) & 15) == 0, "gate_res_f32: 16-byte aligned buffers");
  const long nq = (long)M * (D / 4);
  hipLaunchKernelGGL(f32t::gate_res_f32_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, res, f, gate, gate_ld,
                     rows_per_sample, out, nq, D / 4);
  return mdt_check_launch("gate_res_f32");
}

extern "C" int mdt_gelu_f32(const float* in, float* out, long n, mdt_stream_t stream) {
  MDT_REQUIRE(in && out && n > 0, "gelu_f32: bad arguments");
  hipLaunchKernelGGL(f32t::act_f32_kernel<0>, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, in, in, out, n);
  return mdt_check_launch("gelu_f32");
}

extern "C" int mdt_gelu_bwd_f32(const float* dy, const float* x, float* dx, long n, mdt_stream_t stream) {
  MDT_REQUIRE(dy && x && dx && n > 0, "gelu_bwd_f32: bad arguments");
  hipLaunchKernelGGL(f32t::act_f32_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, n);
  return mdt_check_launch("gelu_bwd_f32");
}

extern "C" int mdt_silu_bwd_f32(const float* dy, const float* x, float* dx, long n, mdt_stream_t stream) {
  MDT_REQUIRE(dy && x && dx && n > 0, "silu_bwd_f32: bad arguments");
  hipLaunchKernelGGL(f32t::act_f32_kernel<2>, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, n);
  return mdt_check_launch("silu_bwd_f32");
}

// Backward of timm Attention (call site models/maskdit.py:178) on the packed fp32 qkv buffer [B * L, 3 * H * hd]:
// P = softmax(q k^T hd^-0.5) is recomputed, dP = dO v^T, dS = hd^-0.5 P o (dP - rowsum(P o dP)), dq = dS k, dk = dS^T q,
// dv = P^T dO.  Workspace: P and dP / dS (B H L^2 floats each) + what the two transposed products need.
static long attn_bwd_tn_ws(int B, int L, int H, int hd) { return mdt_gemm_f32_tn_ws_floats(L, L, hd, B * H); }

extern "C" long mdt_attn_f32_bwd_ws_floats(int B, int L, int H, int hd) {
  if (B <= 0 || L <= 0 || H <= 0 || hd <= 0) return 0;
  return 2L * B * H * L * L + attn_bwd_tn_ws(B, L, H, hd);
}

extern "C" int mdt_attn_f32_bwd(const float* qkv, const float* dout, float* ws, long ws_floats, float* dqkv, int B, int L, int H,
                                int hd, mdt_stream_t stream) {
  MDT_REQUIRE(qkv && dout && ws && dqkv, "attn_f32_bwd: null pointer");
  MDT_REQUIRE(B > 0 && L > 0 && H > 0 && hd > 0 && hd % 4 == 0 && L % 4 == 0, "attn_f32_bwd: B, L, H, hd > 0; L and hd multiples of 4");
  MDT_REQUIRE((((uintptr_t)qkv | (uintptr_t)dout | (uintptr_t)ws | (uintptr_t)dqkv) & 15) == 0, "attn_f32_bwd: 16-byte aligned buffers");
  MDT_REQUIRE((long)B * H <= 65535, "attn_f32_bwd: batch * heads must not exceed 65535");
  MDT_REQUIRE(ws_floats >= mdt_attn_f32_bwd_ws_floats(B, L, H, hd), "attn_f32_bwd: workspace smaller than mdt_attn_f32_bwd_ws_floats()");
  const long W = (long)H * hd, LL = (long)L * L, SS = (long)B * H * LL;
  float* P = ws;
  float* dP = ws + SS;
  float* tnws = ws + 2 * SS;
  const long tnws_floats = attn_bwd_tn_ws(B, L, H, hd);
  const float scale = 1.f / sqrtf((float)hd);
  int rc;
  mdt_gemm_f32_args g = {};
  // P = softmax(q k^T * scale)
  g.A = qkv; g.lda = 3 * W; g.B = qkv + W; g.ldb = 3 * W; g.b_kmajor = 0;
  g.M = L; g.N = L; g.K = hd; g.epi = MDT_F32EPI_NONE;
  g.out = P; g.ldo = L; g.batch = B * H; g.heads = H;
  g.a_stride_b = L * 3 * W; g.a_stride_h = hd; g.b_stride_b = L * 3 * W; g.b_stride_h = hd;
  g.o_stride_b = H * LL; g.o_stride_h = LL;
  if ((rc = mdt_gemm_f32(&g, stream)) != MDT_OK) return rc;
  if ((rc = mdt_softmax_rows_f32(P, (long)B * H * L, L, L, scale, stream)) != MDT_OK) return rc;
  // dP = dO v^T
  g.A = dout; g.lda = W; g.B = qkv + 2 * W; g.ldb = 3 * W;
  g.out = dP;
  g.a_stride_b = L * W; g.a_stride_h = hd;
  if ((rc = mdt_gemm_f32(&g, stream)) != MDT_OK) return rc;
  // dS in place of dP
  hipLaunchKernelGGL(f32t::attn_ds_rows_f32_kernel, dim3(cdiv((long)B * H * L, 4)), dim3(256), 0, (hipStream_t)stream, P, dP,
                     (long)B * H * L, L, scale);
  if ((rc = mdt_check_launch("attn_f32_bwd (dS)")) != MDT_OK) return rc;
  // dq = dS k   (k rows are the K-major operand)
  mdt_gemm_f32_args q = {};
  q.A = dP; q.lda = L; q.B = qkv + W; q.ldb = 3 * W; q.b_kmajor = 1;
  q.M = L; q.N = hd; q.K = L; q.epi = MDT_F32EPI_NONE;
  q.out = dqkv; q.ldo = 3 * W; q.batch = B * H; q.heads = H;
  q.a_stride_b = H * LL; q.a_stride_h = LL; q.b_stride_b = L * 3 * W; q.b_stride_h = hd;
  q.o_stride_b = L * 3 * W; q.o_stride_h = hd;
  if ((rc = mdt_gemm_f32(&q, stream)) != MDT_OK) return rc;
  // dk = dS^T q, dv = P^T dO
  mdt_gemm_f32_tn_args t = {};
  t.A = dP; t.lda = L; t.B = qkv; t.ldb = 3 * W;
  t.M = L; t.N1 = L; t.N2 = hd;
  t.C = dqkv + W; t.ldc = 3 * W; t.accumulate = 0;
  t.batch = B * H; t.heads = H;
  t.a_stride_b = H * LL; t.a_stride_h = LL; t.b_stride_b = L * 3 * W; t.b_stride_h = hd;
  t.c_stride_b = L * 3 * W; t.c_stride_h = hd;
  t.ws = tnws_floats ? tnws : nullptr; t.ws_floats = tnws_floats;
  if ((rc = mdt_gemm_f32_tn(&t, stream)) != MDT_OK) return rc;
  t.A = P; t.B = dout; t.ldb = W;
  t.b_stride_b = L * W; t.b_stride_h = hd;
  t.C = dqkv + 2 * W;
  return mdt_gemm_f32_tn(&t, stream);
}
