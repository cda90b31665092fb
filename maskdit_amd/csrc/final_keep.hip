// FinalLayer + unpatchify of a decoder-less model (use_decoder=False, models/maskdit.py:529-553): the final layer reads
// the ENCODER's rows -- hidden width D up to 1280, and under masking only the kept tokens of each sample -- and its
// result is scattered to the image position of every kept token while removed patches are exactly zero
// (unmask_tokens with a zero mask token, models/maskdit.py:551-553).
//
//   mdt_final_keep_fwd : one wave per IMAGE token j.  r = restore[b, j]; r < L: LayerNorm-modulate row (b, r) of x and
//                        contract it with the p*p*C weight rows; r >= L: store zeros.  Every patch of F is written by
//                        exactly one wave, so F is fully defined without a zeroing launch and padding rows of x
//                        (L <= r < L_pitch) are never read.
//   mdt_final_keep_bwd : two launches.  (1) one wave per row r of x: dx, the two modulation gradients and dbias; rows
//                        L <= r < L_pitch get dx = 0.  (2) dW: one thread per column of x, 16 weight rows per block.
//
// A row is held in registers as NV float4 per lane (NV = ceil(D / 256): 2 .. 5; at D = 384 and 1152 the last slot is
// half populated), so no instantiation needs LDS for the row and the width bound is the register file, not 160 KB.
#include "common.h"
#include "../../include/maskdit_hip.h"

#define FK_MAXD 1280
#define FK_OT 16  // weight rows per block of the dW kernel

// 'nhwpqc->nchpwq' (models/maskdit.py:421-423): element k = (py*p + px)*C + c of token t -> offset inside one image
__device__ __forceinline__ long fk_unpatch(int t, int k, int w, int p, int C, int R) {
  const int th = t / w, tw = t - th * w;
  const int c = k % C, pq = k / C;
  const int py = pq / p, px = pq - py * p;
  return ((long)c * R + th * p + py) * R + tw * p + px;
}

template <int NV>
__global__ __launch_bounds__(256) void final_keep_fwd_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                             const float* __restrict__ scale, int mod_ld,
                                                             const float* __restrict__ W, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ restore, int ids_ld,
                                                             float* __restrict__ F, float* __restrict__ stats, int B, int T,
                                                             int L, int Lp, int D, int C, int p, int w) {
  const int lane = threadIdx.x & 63;
  const long slot = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= (long)B * T) return;
  const int b = (int)(slot / T), j = (int)(slot - (long)b * T);
  const int r = restore ? restore[(long)b * ids_ld + j] : j;
  const int O = p * p * C, R = w * p;
  float* Fb = F + (long)b * C * R * R;
  if (r < 0 || r >= L) {  // removed token: its patch is zero
    for (int k = lane; k < O; k += 64) Fb[fk_unpatch(j, k, w, p, C, R)] = 0.f;
    return;
  }
  const long row = (long)b * Lp + r;
  const int nv = D >> 2;
  const float* xr = x + row * D;
  f32x4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < nv) {
      v[i] = *(const f32x4*)(xr + 4 * c);
      s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (lane + 64 * i < nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[i][e] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-6f);
  const float* sh = shift + (long)b * mod_ld;
  const float* sc = scale + (long)b * mod_ld;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) {
      const f32x4 a = *(const f32x4*)(sh + 4 * c), m = *(const f32x4*)(sc + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = (v[i][e] - mean) * rstd * (1.f + m[e]) + a[e];
    }
  }
  for (int k0 = 0; k0 < O; k0 += 64) {  // lane kk keeps output k0 + kk
    const int kn = min(64, O - k0);
    float outv = 0.f;
    for (int kk = 0; kk < kn; ++kk) {
      const float* wr = W + (long)(k0 + kk) * D;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
          const f32x4 wv = *(const f32x4*)(wr + 4 * c);
          acc += v[i][0] * wv[0] + v[i][1] * wv[1] + v[i][2] * wv[2] + v[i][3] * wv[3];
        }
      }
      acc = wave_sum(acc);
      if (lane == kk) outv = acc + bias[k0 + kk];
    }
    if (lane < kn) Fb[fk_unpatch(j, k0 + lane, w, p, C, R)] = outv;
  }
  if (lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
}

// grid (B, row chunks over L_pitch); 4 waves, one wave per row.  Stores dx; adds dbias, dshift[b], dscale[b].
template <int NV>
__global__ __launch_bounds__(256) void final_keep_bwd_dx_kernel(const float* __restrict__ dF, const float* __restrict__ x,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ scale, int mod_ld,
                                                                const float* __restrict__ W,
                                                                const int32_t* __restrict__ shuffle, int ids_ld,
                                                                float* __restrict__ dx, float* __restrict__ dbias,
                                                                float* __restrict__ dshift, float* __restrict__ dscale,
                                                                int dmod_ld, int T, int L, int Lp, int chunk, int D, int C,
                                                                int p, int w) {
  __shared__ float red[4 * FK_MAXD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int r_begin = blockIdx.y * chunk, r_end = min(r_begin + chunk, Lp);
  const int nv = D >> 2, O = p * p * C, R = w * p;
  const float* sc = scale + (long)b * mod_ld;
  const float* dFb = dF + (long)b * C * R * R;
  f32x4 scv[NV], a_sh[NV], a_sc[NV];
  float a_b[4] = {0.f, 0.f, 0.f, 0.f};  // lane accumulates dbias[lane + 64 m]
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    scv[i] = a_sh[i] = a_sc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < nv) {
      const f32x4 m = *(const f32x4*)(sc + 4 * c);
      scv[i] = (f32x4){1.f + m[0], 1.f + m[1], 1.f + m[2], 1.f + m[3]};
    }
  }
  const float invD = 1.f / (float)D;
  for (int r = r_begin + wave; r < r_end; r += 4) {
    const long row = (long)b * Lp + r;
    if (r >= L) {  // padding row of the encoder: no gradient flows into it
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) *(f32x4*)(dx + row * D + 4 * c) = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      continue;
    }
    int j = shuffle ? shuffle[(long)b * ids_ld + r] : r;
    j = min(max(j, 0), T - 1);
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float dok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m;
      dok[m] = 0.f;
      if (k < O) {
        dok[m] = dFb[fk_unpatch(j, k, w, p, C, R)];
        a_b[m] += dok[m];
      }
    }
    f32x4 xh[NV], dxn[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      xh[i] = dxn[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c < nv) {
        const f32x4 xv = *(const f32x4*)(x + row * D + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) xh[i][e] = (xv[e] - mean) * rstd;
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (64 * m < O) {
        const int kn = min(64, O - 64 * m);
        for (int kk = 0; kk < kn; ++kk) {
          const float g = __shfl(dok[m], kk, 64);
          const float* wr = W + (long)(64 * m + kk) * D;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
              const f32x4 wv = *(const f32x4*)(wr + 4 * c);
#pragma unroll
              for (int e = 0; e < 4; ++e) dxn[i][e] += g * wv[e];
            }
          }
        }
      }
    }
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (lane + 64 * i < nv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a_sh[i][e] += dxn[i][e];
          a_sc[i][e] += dxn[i][e] * xh[i][e];
          const float gm = dxn[i][e] * scv[i][e];
          dxn[i][e] = gm;
          c1 += gm;
          c2 += gm * xh[i][e];
        }
      }
    }
    c1 = wave_sum(c1) * invD;
    c2 = wave_sum(c2) * invD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (dxn[i][e] - c1 - xh[i][e] * c2);
        *(f32x4*)(dx + row * D + 4 * c) = o;
      }
    }
  }
  if (r_begin >= L) return;  // (block-uniform) a chunk of padding rows only: nothing to add
  // the four waves' column sums through LDS, then one atomic per column: dshift, then dscale
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) *(f32x4*)(red + wave * FK_MAXD + 4 * c) = pass ? a_sc[i] : a_sh[i];
    }
    __syncthreads();
    float* dst = (pass ? dscale : dshift) + (long)b * dmod_ld;
    for (int c = threadIdx.x; c < D; c += 256)
      atomic_add_f32(dst + c, red[c] + red[FK_MAXD + c] + red[2 * FK_MAXD + c] + red[3 * FK_MAXD + c]);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (lane + 64 * m < O) atomic_add_f32(dbias + lane + 64 * m, a_b[m]);
}

// dW[k, c] += sum over kept rows of dF[row, k] * xn[row, c].  grid (column tiles of 256, row chunks over B * L_pitch,
// tiles of FK_OT weight rows); one thread per column, FK_OT running sums; dF, the statistics and the ids are
// block-uniform reads.
__global__ __launch_bounds__(256) void final_keep_bwd_dw_kernel(const float* __restrict__ dF, const float* __restrict__ x,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ scale, int mod_ld,
                                                                const int32_t* __restrict__ shuffle, int ids_ld,
                                                                float* __restrict__ dW, long rows, int rows_per, int T, int L,
                                                                int Lp, int D, int C, int p, int w) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  const int O = p * p * C, R = w * p;
  const int k0 = blockIdx.z * FK_OT;
  const long row0 = (long)blockIdx.y * rows_per, row1 = min(row0 + (long)rows_per, rows);
  long koff[FK_OT];
  float acc[FK_OT];
#pragma unroll
  for (int kk = 0; kk < FK_OT; ++kk) {
    acc[kk] = 0.f;
    koff[kk] = k0 + kk < O ? fk_unpatch(0, k0 + kk, w, p, C, R) : 0;
  }
  int cur_b = -1;
  float shc = 0.f, scc = 0.f;
  for (long row = row0; row < row1; ++row) {
    const int b = (int)(row / Lp), r = (int)(row - (long)b * Lp);
    if (r >= L) continue;
    if (b != cur_b) {
      cur_b = b;
      shc = shift[(long)b * mod_ld + c];
      scc = 1.f + scale[(long)b * mod_ld + c];
    }
    int j = shuffle ? shuffle[(long)b * ids_ld + r] : r;
    j = min(max(j, 0), T - 1);
    const int th = j / w, tw = j - th * w;
    const float* g = dF + (long)b * C * R * R + (long)th * p * R + tw * p;
    const float xn = (x[row * D + c] - stats[2 * row]) * stats[2 * row + 1] * scc + shc;
#pragma unroll
    for (int kk = 0; kk < FK_OT; ++kk)
      if (k0 + kk < O) acc[kk] += g[koff[kk]] * xn;
  }
#pragma unroll
  for (int kk = 0; kk < FK_OT; ++kk)
    if (k0 + kk < O) atomic_add_f32(dW + (long)(k0 + kk) * D + c, acc[kk]);
}

// ------------------------------------------------------------------------------------------

static inline bool fk_aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// shared domain check; returns the token grid's side (0 = refused, message set)
static int fk_domain(const char* who, int B, int T, int L, int& L_pitch, int D, int C, int p, bool has_ids, int ids_ld,
                     int mod_ld) {
  static char msg[160];
#define FK_REFUSE(cond, text)                      \
  do {                                             \
    if (!(cond)) {                                 \
      snprintf(msg, sizeof msg, "%s: %s", who, text); \
      mdt_set_error(msg);                          \
      return 0;                                    \
    }                                              \
  } while (0)
  if (L_pitch <= 0) L_pitch = L;
  FK_REFUSE(B > 0 && T > 0 && C > 0 && p > 0 && D > 0, "bad shape");
  const int w = (int)(sqrtf((float)T) + 0.5f);
  FK_REFUSE(w * w == T, "the token count must be a square");
  FK_REFUSE(L >= 1 && L <= T && L_pitch >= L, "needs 1 <= L <= T and L_pitch >= L");
  FK_REFUSE(has_ids ? ids_ld >= 2 * T : L == T, "ids == NULL means identity (L == T); ids rows hold 2T entries");
  FK_REFUSE(D <= FK_MAXD, "needs D <= 1280");
  const int O = p * p * C;
  FK_REFUSE(O <= 16 || O == 64 || O == 256, "p*p*C must be <= 16, 64 or 256");
  FK_REFUSE(D % 4 == 0, "needs D a multiple of 4");
  FK_REFUSE(O <= 16 || D % 32 == 0, "p*p*C of 64 / 256 needs D a multiple of 32");
  FK_REFUSE(mod_ld % 4 == 0, "modulation rows must be 16-byte aligned (ld a multiple of 4)");
#undef FK_REFUSE
  return w;
}

#define FK_DISPATCH(D, CALL)  \
  do {                        \
    if ((D) <= 512) { CALL(2); }       \
    else if ((D) <= 768) { CALL(3); }  \
    else if ((D) <= 1024) { CALL(4); } \
    else { CALL(5); }                  \
  } while (0)

extern "C" int mdt_final_keep_fwd(const float* x, const float* shift, const float* scale, int mod_ld, const float* W,
                                  const float* bias, const int32_t* ids, int ids_ld, float* F, float* stats, int B, int T,
                                  int L, int L_pitch, int D, int C, int p, mdt_stream_t stream) {
  MDT_REQUIRE(x && shift && scale && W && bias && F && stats, "final_keep_fwd: null pointer");
  const int w = fk_domain("final_keep_fwd", B, T, L, L_pitch, D, C, p, ids != nullptr, ids_ld, mod_ld);
  if (!w) return MDT_ERR_ARG;
  MDT_REQUIRE(fk_aligned16(x) && fk_aligned16(shift) && fk_aligned16(scale) && fk_aligned16(W),
              "final_keep_fwd: x, shift, scale and W must be 16-byte aligned");
  const int32_t* restore = ids ? ids + T : nullptr;  // the second half of an ids row
  const dim3 grid(cdiv((long)B * T, 4));
#define FK_FWD(NV)                                                                                                       \
  hipLaunchKernelGGL(final_keep_fwd_kernel<NV>, grid, dim3(256), 0, (hipStream_t)stream, x, shift, scale, mod_ld, W, bias, \
                     restore, ids_ld, F, stats, B, T, L, L_pitch, D, C, p, w)
  FK_DISPATCH(D, FK_FWD);
#undef FK_FWD
  return mdt_check_launch("final_keep_fwd");
}

extern "C" int mdt_final_keep_bwd(const float* dF, const float* x, const float* stats, const float* shift,
                                  const float* scale, int mod_ld, const float* W, const int32_t* ids, int ids_ld, float* dx,
                                  float* dW, float* dbias, float* dshift, float* dscale, int dmod_ld, int B, int T, int L,
                                  int L_pitch, int D, int C, int p, mdt_stream_t stream) {
  MDT_REQUIRE(dF && x && stats && shift && scale && W && dx && dW && dbias && dshift && dscale,
              "final_keep_bwd: null pointer");
  const int w = fk_domain("final_keep_bwd", B, T, L, L_pitch, D, C, p, ids != nullptr, ids_ld, mod_ld);
  if (!w) return MDT_ERR_ARG;
  MDT_REQUIRE(fk_aligned16(x) && fk_aligned16(scale) && fk_aligned16(W) && fk_aligned16(dx),
              "final_keep_bwd: x, scale, W and dx must be 16-byte aligned");
  const int32_t* shuffle = ids;  // the first half of an ids row
  const int Lp = L_pitch;
  int splits = 1;
  while (B * splits < 1024 && Lp / (splits * 2) >= 16) splits *= 2;
  const int chunk = cdiv(Lp, splits);
  const dim3 grid(B, cdiv(Lp, chunk));
#define FK_BWD(NV)                                                                                                          \
  hipLaunchKernelGGL(final_keep_bwd_dx_kernel<NV>, grid, dim3(256), 0, (hipStream_t)stream, dF, x, stats, scale, mod_ld, W, \
                     shuffle, ids_ld, dx, dbias, dshift, dscale, dmod_ld, T, L, Lp, chunk, D, C, p, w)
  FK_DISPATCH(D, FK_BWD);
#undef FK_BWD
  int rc = mdt_check_launch("final_keep_bwd (dx)");
  if (rc != MDT_OK) return rc;
  const int O = p * p * C;
  const long rows = (long)B * Lp;
  const int gx = cdiv(D, 256), gz = cdiv(O, FK_OT);
  long ny = 2048 / ((long)gx * gz);
  if (ny > rows / 16) ny = rows / 16;
  if (ny < 1) ny = 1;
  if (ny > 65535) ny = 65535;
  const int rows_per = cdiv(rows, ny);
  hipLaunchKernelGGL(final_keep_bwd_dw_kernel, dim3(gx, cdiv(rows, rows_per), gz), dim3(256), 0, (hipStream_t)stream, dF, x,
                     stats, shift, scale, mod_ld, shuffle, ids_ld, dW, rows, rows_per, T, L, Lp, D, C, p, w);
  return mdt_check_launch("final_keep_bwd (dW)");
}
