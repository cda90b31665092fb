// The token boundary of the DiT-*/4 and DiT-*/8 models: tokenizer, de-tokenizer and the patch-pooled loss for patch vectors
// of C * p * p = 64 and 256 elements (C = 4).  The forms of embed.hip / loss.hip are written for 16 elements (per-thread
// accumulator arrays, one lane per output); here the products run on v_mfma_f32_32x32x2_f32 -- exact fp32 products and
// sums, the instruction of f32path.hip -- because the same entries feed the bf16 training plan, the 'fp32' / 'bf16x3'
// inference plans and the fp32 training plan.
//
// Reference: timm PatchEmbed as Conv2d(k=s=p) (models/maskdit.py:278,475), mask_out_token (:116-127), FinalLayer
// (:216-234), unpatchify (:411-424), EDMLoss / mae_loss / patchify (train_utils/loss.py:28-101).
//
// Two product kernels serve the five products:
//   rows_nt_kernel  out[rows, N] = A[rows, K] * W^T, A built in LDS by the workgroup (TM rows): the gathered patch vectors
//                   (tokenizer forward), the LayerNorm-modulated rows (de-tokenizer forward) or the gathered dF patches
//                   (de-tokenizer data gradient, W read K-major).  A wave owns 32-column blocks of N; the weights come
//                   straight from L2 (<= 1.2 MB).  The contraction index is permuted: lane half h of a fragment walks
//                   k in [h K/2, (h + 1) K/2) four at a time (one 16-byte read feeds four MFMAs); A and W use the same
//                   permutation, so the sum is over all K.
//   rows_tn_kernel  dW += X^T * P over a chunk of rows: X[row, d] read from HBM (dout, or the recomputed LayerNorm-modulate
//                   row), P[row, k] the patch vectors gathered into LDS 32 rows at a time.  A wave owns 32 values of d and
//                   all K / 32 column blocks (8 accumulator blocks at K = 256); one fp32 atomic per element and chunk, as
//                   the 16-element kernels do.
// Every barrier is a full __syncthreads and every wait is the compiler's: nothing is hand-counted in this file.
#include "patch_wide.h"
#include "../../include/maskdit_hip.h"

typedef __attribute__((ext_vector_type(16))) float pw_f32x16;

namespace pw {

enum { NT_TOKENIZE = 0, NT_FINAL = 1, NT_FINAL_DGRAD = 2 };
enum { TN_TOKENIZE = 0, TN_FINAL = 1 };

// element e of a patch in IMAGE order (c, py, px): offset inside one sample's [C, R, R] image
__device__ __forceinline__ long patch_off(int t, int e, int w, int p, int R, int& c, int& py, int& px) {
  const int p2 = p * p;
  c = e / p2;
  const int rem = e - c * p2;
  py = rem / p;
  px = rem - py * p;
  const int th = t / w, tw = t - th * w;
  return ((long)c * R + th * p + py) * R + tw * p + px;
}

// offset of output k of the de-tokenizer, 'nhwpqc->nchpwq' (models/maskdit.py:421-423): k = (py * p + px) * C + c
__device__ __forceinline__ long unpatch_off(int t, int k, int w, int p, int C, int R) {
  const int c = k % C, pq = k / C, py = pq / p, px = pq - py * p;
  const int th = t / w, tw = t - th * w;
  return ((long)c * R + th * p + py) * R + tw * p + px;
}

struct NTParams {
  const float* src;       // x image / residual-stream rows / dF image
  const float* in_scale;  // tokenizer: optional per-sample factor
  const int32_t* ids;     // tokenizer: optional kept-token table
  int ids_ld;
  const float* W;         // [N, K]  (NT_FINAL_DGRAD: [K, N])
  const float* bias;
  const float* pos;       // tokenizer: [T, N]
  const float* shift;     // de-tokenizer forward: modulation rows
  const float* scale;
  int mod_ld;
  float* out;             // [rows, N] (NT_FINAL: F [B, C, R, R])
  float* stats;           // NT_FINAL: (mean, rstd) per row
  long nrows;
  int L;                  // rows per sample
  int K, N, C, R, p;
};

template <int MODE, int TM>
__global__ __launch_bounds__(256) void rows_nt_kernel(NTParams P) {
  extern __shared__ float lds[];  // [TM][K + 4]
  __shared__ int tok[TM];
  const int K = P.K, N = P.N, ldk = K + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * TM;
  const int w = P.R / P.p;
  const long img = (long)P.C * P.R * P.R;
  if (MODE == NT_FINAL) {
    // LayerNorm (eps 1e-6, biased variance) + modulate, one wave per row, K = Dd <= 512: two float4 per lane
    const int nv = K >> 2;
    for (int tj = wave; tj < TM; tj += 4) {
      const long row = row0 + tj;
      f32x4 v[2];
      v[0] = v[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (row < P.nrows) {  // (wave-uniform)
        const int b = (int)(row / P.L);
        const float* xr = P.src + row * K;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int c = lane + 64 * i;
          if (c < nv) {
            v[i] = *(const f32x4*)(xr + 4 * c);
            s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
          }
        }
        const float mean = wave_sum(s) / (float)K;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int c = lane + 64 * i;
          if (c < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = v[i][e] - mean;
              q += d * d;
            }
          }
        }
        const float rstd = rsqrtf(wave_sum(q) / (float)K + 1e-6f);
        const float* sh = P.shift + (long)b * P.mod_ld;
        const float* sc = P.scale + (long)b * P.mod_ld;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int c = lane + 64 * i;
          if (c < nv) {
            const f32x4 a = *(const f32x4*)(sh + 4 * c), m = *(const f32x4*)(sc + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = (v[i][e] - mean) * rstd * (1.f + m[e]) + a[e];
          }
        }
        if (lane == 0) {
          P.stats[2 * row] = mean;
          P.stats[2 * row + 1] = rstd;
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) *(f32x4*)(lds + tj * ldk + 4 * c) = v[i];
      }
    }
  } else {
    // gather the patch vectors of TM rows: consecutive threads walk one patch in image order (px fastest)
    for (int idx = threadIdx.x; idx < TM * K; idx += 256) {
      const int tj = idx / K, e = idx - tj * K;
      const long row = row0 + tj;
      float val = 0.f;
      int c, py, px;
      int kpos = e;
      if (row < P.nrows) {
        const int b = (int)(row / P.L), j = (int)(row - (long)b * P.L);
        const int t = (MODE == NT_TOKENIZE && P.ids) ? P.ids[(long)b * P.ids_ld + j] : j;
        const long off = patch_off(t, e, w, P.p, P.R, c, py, px);
        val = P.src[(long)b * img + off];
        if (MODE == NT_TOKENIZE) {
          if (P.in_scale) val *= P.in_scale[b];
          if (e == 0) tok[tj] = t;
        } else {
          kpos = (py * P.p + px) * P.C + c;
        }
      } else if (MODE == NT_FINAL_DGRAD) {
        patch_off(0, e, w, P.p, P.R, c, py, px);
        kpos = (py * P.p + px) * P.C + c;
      }
      lds[tj * ldk + kpos] = val;
    }
  }
  __syncthreads();
  const int r = lane & 31, h = lane >> 5, Kh = K >> 1;
  const float* a0p = lds + r * ldk + h * Kh;
  const float* a1p = lds + (32 + r) * ldk + h * Kh;
  for (int ct = wave; ct * 32 < N; ct += 4) {
    const int col = ct * 32 + r;  // N is a multiple of 32 (host check)
    pw_f32x16 acc0, acc1;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc0[v] = acc1[v] = 0.f;
    for (int s = 0; s < Kh; s += 4) {
      f32x4 b4;
      if (MODE == NT_FINAL_DGRAD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b4[e] = P.W[(long)(h * Kh + s + e) * N + col];
      } else {
        b4 = *(const f32x4*)(P.W + (long)col * K + h * Kh + s);
      }
      const f32x4 a0 = *(const f32x4*)(a0p + s);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b4[e], acc0, 0, 0, 0);
      if (TM == 64) {
        const f32x4 a1 = *(const f32x4*)(a1p + s);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b4[e], acc1, 0, 0, 0);
      }
    }
    const float bv = MODE == NT_FINAL_DGRAD ? 0.f : P.bias[col];
#pragma unroll
    for (int half = 0; half < TM / 32; ++half) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int tj = half * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
        const long row = row0 + tj;
        if (row >= P.nrows) continue;
        const float a = half ? acc1[v] : acc0[v];
        if (MODE == NT_TOKENIZE) {
          P.out[row * N + col] = a + bv + P.pos[(long)tok[tj] * N + col];
        } else if (MODE == NT_FINAL) {
          const int b = (int)(row / P.L), t = (int)(row - (long)b * P.L);
          P.out[(long)b * img + unpatch_off(t, col, w, P.p, P.C, P.R)] = a + bv;
        } else {
          P.out[row * N + col] = a;
        }
      }
    }
  }
}

struct TNParams {
  const float* xsrc;      // dout [rows, ND] / residual-stream rows x [rows, ND]
  const float* stats;     // TN_FINAL: (mean, rstd) per row
  const float* shift;
  const float* scale;
  int mod_ld;
  const float* img;       // x image / dF image
  const float* in_scale;
  const int32_t* ids;
  int ids_ld;
  float* dW;              // TN_TOKENIZE: [ND, NK]; TN_FINAL: [NK, ND]
  float* dbias;           // TN_TOKENIZE: [ND]; TN_FINAL: [NK]
  long nrows;
  int chunk;              // rows per workgroup (multiple of 32)
  int L, ND, C, R, p;
};

// NB = NK / 32 column blocks (NK = C * p * p = 64 or 256)
template <int MODE, int NB>
__global__ __launch_bounds__(256) void rows_tn_kernel(TNParams P) {
  constexpr int NK = NB * 32, LDP = NK + 32;  // (+32: the two lane halves of a fragment read rows 2s and 2s + 1 from different bank halves)
  extern __shared__ float pv[];               // [32][LDP]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int w = P.R / P.p;
  const long img = (long)P.C * P.R * P.R;
  const int dbase = blockIdx.y * 128 + wave * 32;
  const bool wvalid = dbase < P.ND;  // ND is a multiple of 32 (host check): a wave is valid or idle as a whole
  const int d = dbase + r;
  const long rbeg = (long)blockIdx.x * P.chunk, rend = min(rbeg + (long)P.chunk, P.nrows);
  pw_f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
  float ab = 0.f;  // TN_TOKENIZE: bias gradient of column d (this lane's row parity); TN_FINAL: of output threadIdx.x
  for (long t0 = rbeg; t0 < rend; t0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * NK; idx += 256) {
      const int tj = idx / NK, e = idx - tj * NK;
      const long row = t0 + tj;
      int c, py, px;
      float val = 0.f;
      const int b = (int)(min(row, P.nrows - 1) / P.L), j = (int)(min(row, P.nrows - 1) - (long)b * P.L);
      const int t = (MODE == TN_TOKENIZE && P.ids) ? P.ids[(long)b * P.ids_ld + j] : j;
      const long off = patch_off(t, e, w, P.p, P.R, c, py, px);
      if (row < rend) {
        val = P.img[(long)b * img + off];
        if (MODE == TN_TOKENIZE && P.in_scale) val *= P.in_scale[b];
      }
      const int kpos = MODE == TN_TOKENIZE ? e : (py * P.p + px) * P.C + c;
      pv[tj * LDP + kpos] = val;
    }
    __syncthreads();
    if (MODE == TN_FINAL && blockIdx.y == 0 && threadIdx.x < NK) {
      float s = 0.f;
#pragma unroll 8
      for (int tj = 0; tj < 32; ++tj) s += pv[tj * LDP + threadIdx.x];
      ab += s;
    }
    if (!wvalid) continue;
    float av[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const long row = t0 + 2 * s + h;
      float a = 0.f;
      if (row < rend) {
        a = P.xsrc[row * P.ND + d];
        if (MODE == TN_FINAL) {
          const int b = (int)(row / P.L);
          const float mean = P.stats[2 * row], rstd = P.stats[2 * row + 1];
          a = (a - mean) * rstd * (1.f + P.scale[(long)b * P.mod_ld + d]) + P.shift[(long)b * P.mod_ld + d];
        }
      }
      av[s] = a;
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (MODE == TN_TOKENIZE) ab += av[s];
      const float* prow = pv + (2 * s + h) * LDP + r;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const float bvv = prow[j * 32];
        // TN_TOKENIZE: block rows = d, columns = k; TN_FINAL: block rows = o, columns = d (dW is [NK, ND])
        acc[j] = MODE == TN_TOKENIZE ? __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bvv, acc[j], 0, 0, 0)
                                     : __builtin_amdgcn_mfma_f32_32x32x2f32(bvv, av[s], acc[j], 0, 0, 0);
      }
    }
  }
  if (MODE == TN_FINAL && blockIdx.y == 0 && threadIdx.x < NK) atomic_add_f32(P.dbias + threadIdx.x, ab);
  if (!wvalid) return;
  if (MODE == TN_TOKENIZE) {
    ab += __shfl_xor(ab, 32, 64);
    if (h == 0) atomic_add_f32(P.dbias + d, ab);
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int i = 8 * (v >> 2) + 4 * h + (v & 3);
      if (MODE == TN_TOKENIZE) atomic_add_f32(P.dW + (long)(dbase + i) * NK + j * 32 + r, acc[j][v]);
      else atomic_add_f32(P.dW + (long)(j * 32 + i) * P.ND + d, acc[j][v]);
    }
  }
}

// LayerNorm-modulate backward of the de-tokenizer, in place: dx holds dxn = dO W on entry.  grid (B, chunks), a wave per
// token; dshift[b] += sum dxn, dscale[b] += sum dxn * xhat.  Dd <= 512.
__global__ __launch_bounds__(256) void final_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                           const float* __restrict__ scale, int mod_ld, float* __restrict__ dx,
                                                           float* __restrict__ dshift, float* __restrict__ dscale, int dmod_ld,
                                                           int T, int chunk, int Dd) {
  extern __shared__ float red[];  // [4 waves][2 * Dd]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int t_begin = blockIdx.y * chunk, t_end = min(t_begin + chunk, T);
  const int nv = Dd >> 2;
  const float* sc = scale + (long)b * mod_ld;
  f32x4 scv[2], a_sh[2], a_sc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i;
    scv[i] = a_sh[i] = a_sc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < nv) {
      const f32x4 m = *(const f32x4*)(sc + 4 * c);
      scv[i] = (f32x4){1.f + m[0], 1.f + m[1], 1.f + m[2], 1.f + m[3]};
    }
  }
  const float invD = 1.f / (float)Dd;
  for (int t = t_begin + wave; t < t_end; t += 4) {
    const long row = (long)b * T + t;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    f32x4 xh[2], g[2];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      xh[i] = g[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c < nv) {
        const f32x4 xv = *(const f32x4*)(x + row * Dd + 4 * c);
        g[i] = *(const f32x4*)(dx + row * Dd + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xh[i][e] = (xv[e] - mean) * rstd;
          a_sh[i][e] += g[i][e];
          a_sc[i][e] += g[i][e] * xh[i][e];
          const float gm = g[i][e] * scv[i][e];
          g[i][e] = gm;
          c1 += gm;
          c2 += gm * xh[i][e];
        }
      }
    }
    c1 = wave_sum(c1) * invD;
    c2 = wave_sum(c2) * invD;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (g[i][e] - c1 - xh[i][e] * c2);
        *(f32x4*)(dx + row * Dd + 4 * c) = o;
      }
    }
  }
  float* mine = red + (long)wave * 2 * Dd;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) {
      *(f32x4*)(mine + 4 * c) = a_sh[i];
      *(f32x4*)(mine + Dd + 4 * c) = a_sc[i];
    }
  }
  __syncthreads();
  const int tot = 2 * Dd;
  for (int idx = threadIdx.x; idx < tot; idx += 256) {
    const float s4 = red[idx] + red[tot + idx] + red[2 * tot + idx] + red[3 * tot + idx];
    if (idx < Dd) atomic_add_f32(dshift + (long)b * dmod_ld + idx, s4);
    else atomic_add_f32(dscale + (long)b * dmod_ld + idx - Dd, s4);
  }
}

// ---- loss: a wave per patch, NPL = n / 64 elements per lane -------------------------------------------------------------
// grid (B); the four waves of a workgroup walk the T patches of one sample, thread 0 forms the sample's loss
template <int NPL>
__global__ __launch_bounds__(256) void edm_loss_fwd_kernel(const float* __restrict__ F, const float* __restrict__ yn,
                                                           const float* __restrict__ y, const float* __restrict__ coef,
                                                           const float* __restrict__ mask, float mae_coef,
                                                           float* __restrict__ D, float* __restrict__ loss, int C, int R, int p) {
  __shared__ float sm[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, B = gridDim.x;
  const int w = R / p, T = w * w;
  constexpr int n = 64 * NPL;
  const long base = (long)b * C * R * R;
  const float c_skip = coef[b], c_out = coef[(long)B + b], wgt = coef[4L * B + b];
  float s_edm = 0.f, s_mae = 0.f, n_un = 0.f;  // wave-uniform
  for (int t = wave; t < T; t += 4) {
    const float mk = mask ? mask[(long)b * T + t] : 0.f;
    float tv[NPL], dv[NPL];
    float se = 0.f, sum = 0.f;
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
      int c, py, px;
      const long idx = base + patch_off(t, lane + 64 * u, w, p, R, c, py, px);
      const float ynv = yn[idx];
      const float d = c_skip * ynv + c_out * F[idx];
      D[idx] = d;
      const float e = d - y[idx];
      se += e * e;
      sum += ynv;
      tv[u] = ynv;
      dv[u] = d;
    }
    if (mk == 0.f) {
      s_edm += wgt * wave_sum(se) / (float)n;
      n_un += 1.f;
    } else if (mae_coef > 0.f) {
      const float mean = wave_sum(sum) / (float)n;
      float sumsq = 0.f;
#pragma unroll
      for (int u = 0; u < NPL; ++u) sumsq += (tv[u] - mean) * (tv[u] - mean);
      const float inv = rsqrtf(wave_sum(sumsq) / (float)(n - 1) + 1e-6f);
      float sl = 0.f;
#pragma unroll
      for (int u = 0; u < NPL; ++u) {
        const float e = dv[u] - (tv[u] - mean) * inv;
        sl += e * e;
      }
      s_mae += wave_sum(sl) / (float)n;
    }
  }
  if (lane == 0) {
    sm[0][wave] = s_edm;
    sm[1][wave] = s_mae;
    sm[2][wave] = n_un;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float e = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3], m = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
    const float u = sm[2][0] + sm[2][1] + sm[2][2] + sm[2][3];
    float l = e / u;
    if (mask && mae_coef > 0.f) l += mae_coef * m / ((float)T - u);
    loss[b] = l;
  }
}

// grid (B, splits): every workgroup counts the sample's unmasked patches itself, then its waves take patches
// blockIdx.y * 4 + wave, + 4 * splits, ...
template <int NPL>
__global__ __launch_bounds__(256) void edm_loss_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ D,
                                                           const float* __restrict__ yn, const float* __restrict__ y,
                                                           const float* __restrict__ coef, const float* __restrict__ mask,
                                                           float mae_coef, float* __restrict__ dF, int C, int R, int p) {
  __shared__ float sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, B = gridDim.x;
  const int w = R / p, T = w * w;
  constexpr int n = 64 * NPL;
  const long base = (long)b * C * R * R;
  const float c_out = coef[(long)B + b], wgt = coef[4L * B + b];
  float cnt = (float)T;
  if (mask) {
    float cl = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) cl += (mask[(long)b * T + t] == 0.f) ? 1.f : 0.f;
    cl = wave_sum(cl);
    if (lane == 0) sm[wave] = cl;
    __syncthreads();
    cnt = sm[0] + sm[1] + sm[2] + sm[3];
  }
  const float g = dloss[b];
  const float k_edm = g * wgt * 2.f / ((float)n * cnt) * c_out;
  const float k_mae = (mask && mae_coef > 0.f) ? g * mae_coef * 2.f / ((float)n * ((float)T - cnt)) * c_out : 0.f;
  for (int t = blockIdx.y * 4 + wave; t < T; t += 4 * gridDim.y) {
    const float mk = mask ? mask[(long)b * T + t] : 0.f;
    long idx[NPL];
    float tv[NPL];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
      int c, py, px;
      idx[u] = base + patch_off(t, lane + 64 * u, w, p, R, c, py, px);
    }
    if (mk == 0.f) {
#pragma unroll
      for (int u = 0; u < NPL; ++u) dF[idx[u]] = k_edm * (D[idx[u]] - y[idx[u]]);
    } else {
#pragma unroll
      for (int u = 0; u < NPL; ++u) {
        tv[u] = yn[idx[u]];
        sum += tv[u];
      }
      const float mean = wave_sum(sum) / (float)n;
      float sumsq = 0.f;
#pragma unroll
      for (int u = 0; u < NPL; ++u) sumsq += (tv[u] - mean) * (tv[u] - mean);
      const float inv = rsqrtf(wave_sum(sumsq) / (float)(n - 1) + 1e-6f);
#pragma unroll
      for (int u = 0; u < NPL; ++u) dF[idx[u]] = k_mae * (D[idx[u]] - (tv[u] - mean) * inv);
    }
  }
}

// rows_nt_kernel asks for more than 64 KB of dynamic LDS at K = 256 (TM = 64) and at Dd = 512 (TM = 32).  The attribute
// is set to the largest request of the instantiation's domain: the runtime refuses a value that, with the kernel's static
// LDS (tok[]), passes the 160 KB of a workgroup, and a refusal left unread would surface as the next launch's error.
template <typename Kern>
static int allow_lds(Kern k, bool& done, int bytes, const char* what) {
  if (!done) {
    if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      (void)hipGetLastError();
      mdt_set_error(what);
      return MDT_ERR_LAUNCH;
    }
    done = true;
  }
  return 0;
}

enum { NT_LDS_ROWS64 = 64 * (256 + 4) * 4, NT_LDS_ROWS32 = 32 * (512 + 4) * 4 };

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int isqrt_exact(int T) {
  int w = 1;
  while (w * w < T) ++w;
  return w * w == T ? w : 0;
}

}  // namespace pw

using namespace pw;

int mdt_wide_patch_embed_fwd(const float* x, const float* in_scale, const float* W, const float* bias, const float* pos,
                             const int32_t* ids, int ids_ld, float* out, int B, int C, int R, int p, int L, int D,
                             hipStream_t stream) {
  MDT_REQUIRE(B > 0 && L > 0 && D > 0 && D % 32 == 0 && aligned16(W), "patch_embed_fwd: C*p*p of 64 / 256 needs D % 32 == 0 and a 16-byte aligned weight");
  NTParams P{};
  P.src = x; P.in_scale = in_scale; P.ids = ids; P.ids_ld = ids_ld; P.W = W; P.bias = bias; P.pos = pos; P.out = out;
  P.nrows = (long)B * L; P.L = L; P.K = C * p * p; P.N = D; P.C = C; P.R = R; P.p = p;
  static bool attr = false;
  if (int rc = allow_lds(rows_nt_kernel<NT_TOKENIZE, 64>, attr, NT_LDS_ROWS64, "patch_embed_fwd: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed")) return rc;
  const size_t lds = (size_t)64 * (P.K + 4) * sizeof(float);
  hipLaunchKernelGGL((rows_nt_kernel<NT_TOKENIZE, 64>), dim3(cdiv(P.nrows, 64)), dim3(256), lds, stream, P);
  return mdt_check_launch("patch_embed_fwd");
}

static int tn_chunk(long nrows) {
  long c = (nrows + 63) / 64;  // at most 64 chunks: one atomic per element of dW and chunk
  if (c < 512) c = 512;
  return (int)((c + 31) / 32 * 32);
}

int mdt_wide_patch_embed_bwd(const float* x, const float* in_scale, const float* dout, const int32_t* ids, int ids_ld,
                             float* dW, float* dbias, int B, int C, int R, int p, int L, int D, hipStream_t stream) {
  MDT_REQUIRE(B > 0 && L > 0 && D > 0 && D % 32 == 0, "patch_embed_bwd: C*p*p of 64 / 256 needs D % 32 == 0");
  TNParams P{};
  P.xsrc = dout; P.img = x; P.in_scale = in_scale; P.ids = ids; P.ids_ld = ids_ld; P.dW = dW; P.dbias = dbias;
  P.nrows = (long)B * L; P.chunk = tn_chunk(P.nrows); P.L = L; P.ND = D; P.C = C; P.R = R; P.p = p;
  dim3 grid(cdiv(P.nrows, P.chunk), cdiv(D, 128));
  if (C * p * p == 64) {
    hipLaunchKernelGGL((rows_tn_kernel<TN_TOKENIZE, 2>), grid, dim3(256), 32 * (64 + 32) * sizeof(float), stream, P);
  } else {
    hipLaunchKernelGGL((rows_tn_kernel<TN_TOKENIZE, 8>), grid, dim3(256), 32 * (256 + 32) * sizeof(float), stream, P);
  }
  return mdt_check_launch("patch_embed_bwd");
}

int mdt_wide_final_fwd(const float* x, const float* shift, const float* scale, int mod_ld, const float* W, const float* bias,
                       float* F, float* stats, int B, int T, int Dd, int C, int p, hipStream_t stream) {
  const int w = isqrt_exact(T);
  MDT_REQUIRE(B > 0 && w > 0 && Dd % 8 == 0 && Dd <= 512 && mod_ld % 4 == 0 && aligned16(W) && aligned16(x) && aligned16(shift) &&
                  aligned16(scale),
              "final_fwd: p*p*C of 64 / 256 needs a square token grid, Dd % 8 == 0, Dd <= 512 and 16-byte aligned rows");
  NTParams P{};
  P.src = x; P.W = W; P.bias = bias; P.shift = shift; P.scale = scale; P.mod_ld = mod_ld; P.out = F; P.stats = stats;
  P.nrows = (long)B * T; P.L = T; P.K = Dd; P.N = C * p * p; P.C = C; P.R = w * p; P.p = p;
  static bool attr = false;
  if (int rc = allow_lds(rows_nt_kernel<NT_FINAL, 32>, attr, NT_LDS_ROWS32, "final_fwd: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed")) return rc;
  const size_t lds = (size_t)32 * (Dd + 4) * sizeof(float);
  hipLaunchKernelGGL((rows_nt_kernel<NT_FINAL, 32>), dim3(cdiv(P.nrows, 32)), dim3(256), lds, stream, P);
  return mdt_check_launch("final_fwd");
}

int mdt_wide_final_bwd(const float* dF, const float* x, const float* stats, const float* shift, const float* scale, int mod_ld,
                       const float* W, float* dx, float* dW, float* dbias, float* dshift, float* dscale, int dmod_ld, int B,
                       int T, int Dd, int C, int p, hipStream_t stream) {
  const int w = isqrt_exact(T);
  MDT_REQUIRE(B > 0 && w > 0 && Dd % 32 == 0 && Dd <= 512 && mod_ld % 4 == 0 && aligned16(x) && aligned16(dx) && aligned16(scale),
              "final_bwd: p*p*C of 64 / 256 needs a square token grid, Dd % 32 == 0, Dd <= 512 and 16-byte aligned rows");
  const int O = C * p * p;
  // 1. dx <- dO W  (dO = the patches of dF in output order, gathered by the workgroup)
  NTParams Q{};
  Q.src = dF; Q.W = W; Q.out = dx; Q.nrows = (long)B * T; Q.L = T; Q.K = O; Q.N = Dd; Q.C = C; Q.R = w * p; Q.p = p;
  static bool attr = false;
  if (int rc = allow_lds(rows_nt_kernel<NT_FINAL_DGRAD, 64>, attr, NT_LDS_ROWS64, "final_bwd: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed")) return rc;
  hipLaunchKernelGGL((rows_nt_kernel<NT_FINAL_DGRAD, 64>), dim3(cdiv(Q.nrows, 64)), dim3(256),
                     (size_t)64 * (O + 4) * sizeof(float), stream, Q);
  int rc = mdt_check_launch("final_bwd (data gradient)");
  if (rc) return rc;
  // 2. dW += dO^T xn, dbias += colsum(dO): xn is recomputed from x and the saved statistics
  TNParams P{};
  P.xsrc = x; P.stats = stats; P.shift = shift; P.scale = scale; P.mod_ld = mod_ld; P.img = dF; P.dW = dW; P.dbias = dbias;
  P.nrows = (long)B * T; P.chunk = tn_chunk(P.nrows); P.L = T; P.ND = Dd; P.C = C; P.R = w * p; P.p = p;
  dim3 grid(cdiv(P.nrows, P.chunk), cdiv(Dd, 128));
  if (O == 64) {
    hipLaunchKernelGGL((rows_tn_kernel<TN_FINAL, 2>), grid, dim3(256), 32 * (64 + 32) * sizeof(float), stream, P);
  } else {
    hipLaunchKernelGGL((rows_tn_kernel<TN_FINAL, 8>), grid, dim3(256), 32 * (256 + 32) * sizeof(float), stream, P);
  }
  rc = mdt_check_launch("final_bwd (weight gradient)");
  if (rc) return rc;
  // 3. LayerNorm-modulate backward in place over dx; dshift / dscale accumulate
  int splits = 1;
  while (B * splits < 1024 && T / (splits * 2) >= 16) splits *= 2;
  const int chunk = cdiv(T, splits);
  hipLaunchKernelGGL(final_ln_bwd_kernel, dim3(B, cdiv(T, chunk)), dim3(256), (size_t)4 * 2 * Dd * sizeof(float), stream, x,
                     stats, scale, mod_ld, dx, dshift, dscale, dmod_ld, T, chunk, Dd);
  return mdt_check_launch("final_bwd");
}

int mdt_wide_edm_loss_fwd(const float* F, const float* yn, const float* y, const float* coef, const float* mask,
                          float mae_coef, float* D, float* loss, int B, int C, int R, int p, hipStream_t stream) {
  MDT_REQUIRE(B > 0, "edm_loss_fwd: empty batch");
  if (C * p * p == 64) {
    hipLaunchKernelGGL((edm_loss_fwd_kernel<1>), dim3(B), dim3(256), 0, stream, F, yn, y, coef, mask, mae_coef, D, loss, C, R, p);
  } else {
    hipLaunchKernelGGL((edm_loss_fwd_kernel<4>), dim3(B), dim3(256), 0, stream, F, yn, y, coef, mask, mae_coef, D, loss, C, R, p);
  }
  return mdt_check_launch("edm_loss_fwd");
}

int mdt_wide_edm_loss_bwd(const float* dloss, const float* D, const float* yn, const float* y, const float* coef,
                          const float* mask, float mae_coef, float* dF, int B, int C, int R, int p, hipStream_t stream) {
  MDT_REQUIRE(B > 0, "edm_loss_bwd: empty batch");
  const int T = (R / p) * (R / p);
  int splits = 1;
  while (B * splits < 1024 && T / (splits * 2) >= 4) splits *= 2;
  dim3 grid(B, splits);
  if (C * p * p == 64) {
    hipLaunchKernelGGL((edm_loss_bwd_kernel<1>), grid, dim3(256), 0, stream, dloss, D, yn, y, coef, mask, mae_coef, dF, C, R, p);
  } else {
    hipLaunchKernelGGL((edm_loss_bwd_kernel<4>), grid, dim3(256), 0, stream, dloss, D, yn, y, coef, mask, mae_coef, dF, C, R, p);
  }
  return mdt_check_launch("edm_loss_bwd");
}
