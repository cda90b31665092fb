// Fused AdamW + EMA + bf16 weight-shadow refresh over the flat parameter arena, and the
// batched bf16 transposes that keep the K-major (dgrad) weight shadows in sync.
//
// Reference: apex.optimizers.FusedAdam(lr, adam_w_mode=True, weight_decay=0) (train.py:141,226)
// -- Adam with decoupled weight decay and bias correction (torch.optim.AdamW equivalent shown at
// train_wds.py:202) -- and update_ema (train_utils/helper.py:47-58: ema = d*ema + (1-d)*p).
// One pass: 20 B/param read (p, g, m, v, ema) + 18 B/param written (p, m, v, ema, bf16 shadow).
#include "common.h"
#include "../../include/maskdit_hip.h"

static_assert(sizeof(mdt_guard_state) == 64, "mdt_guard_state is a 64-byte record (maskdit_amd/guard.py views it by offset)");

// One element of the AdamW update, shared by the plain and the guarded kernel (`gg` = the already scaled gradient).
struct AdamHyp {
  float lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2;
};
__device__ __forceinline__ void adamw_element(float& pp, float gg, float& mm, float& v2, const AdamHyp& h) {
  pp = pp * (1.f - h.lr * h.wd);
  mm = h.b1 * mm + (1.f - h.b1) * gg;
  v2 = h.b2 * v2 + (1.f - h.b2) * gg * gg;
  float denom = sqrtf(v2) * h.inv_sqrt_bc2 + h.eps;
  pp -= (h.lr * h.inv_bc1) * (mm / denom);
}

// GUARDED: `gs` (mdt_guard_state, written by guard_decide_kernel earlier on the stream) supplies the clip coefficient,
// the skip decision and -- with device_bc -- the bias corrections of the device's applied-step count.  On skip the grid
// does the EMA update alone and writes neither p, m, v nor the bf16 shadow.
template <bool GUARDED>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, bf16* __restrict__ w16, long n4,
                                                        long n, float lr, float b1, float b2, float eps, float wd,
                                                        float inv_bc1, float inv_sqrt_bc2, float ema_decay,
                                                        float gscale, const mdt_guard_state* __restrict__ gs,
                                                        int device_bc) {
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (GUARDED) {
    const mdt_guard_state st = *gs;  // (one 64-byte read per thread, the same line for the whole grid)
    if (st.skip) {
      if (!ema) return;
      for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 pv = *(const f32x4*)(p + 4 * i);
        f32x4 ev = *(const f32x4*)(ema + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[e] = ema_decay * ev[e] + (1.f - ema_decay) * pv[e];
        *(f32x4*)(ema + 4 * i) = ev;
      }
      if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        long i = (n4 << 2) + threadIdx.x;
        ema[i] = ema_decay * ema[i] + (1.f - ema_decay) * p[i];
      }
      return;
    }
    gscale *= st.coef;
    if (device_bc) {
      inv_bc1 = st.inv_bc1;
      inv_sqrt_bc2 = st.inv_sqrt_bc2;
    }
  }
  const AdamHyp h = {lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2};
  // two float4 per array and iteration: ten 16-byte loads in flight per lane before the first use
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const long i1 = i0 + stride;
    const bool two = i1 < n4;
    const long ix[2] = {i0, two ? i1 : i0};
    f32x4 pv[2], gv[2], mv[2], vv[2], ev[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      pv[u] = *(const f32x4*)(p + 4 * ix[u]);
      gv[u] = *(const f32x4*)(g + 4 * ix[u]);
      mv[u] = *(const f32x4*)(m + 4 * ix[u]);
      vv[u] = *(const f32x4*)(v + 4 * ix[u]);
      ev[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ema) ev[u] = *(const f32x4*)(ema + 4 * ix[u]);  // (wave-uniform)
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      bf16x4 sh;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pp = pv[u][e], mm = mv[u][e], v2 = vv[u][e];
        adamw_element(pp, gv[u][e] * gscale, mm, v2, h);
        pv[u][e] = pp; mv[u][e] = mm; vv[u][e] = v2;
        sh[e] = f2bf(pp);
      }
      const long i = ix[u];
      *(f32x4*)(p + 4 * i) = pv[u];
      *(f32x4*)(m + 4 * i) = mv[u];
      *(f32x4*)(v + 4 * i) = vv[u];
      if (ema) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[u][e] = ema_decay * ev[u][e] + (1.f - ema_decay) * pv[u][e];
        *(f32x4*)(ema + 4 * i) = ev[u];
      }
      if (w16) *(bf16x4*)(w16 + 4 * i) = sh;
    }
  }
  // tail (n % 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    long i = (n4 << 2) + threadIdx.x;
    float pp = p[i], mm = m[i], v2 = v[i];
    adamw_element(pp, g[i] * gscale, mm, v2, h);
    p[i] = pp; m[i] = mm; v[i] = v2;
    if (ema) ema[i] = ema_decay * ema[i] + (1.f - ema_decay) * pp;
    if (w16) w16[i] = f2bf(pp);
  }
}

// ---- gradient guard: ordered fp64 sum of squares -> decision (skip / clip coefficient) ------------------------------
// Stage 1: workgroup c owns elements [c * chunk, min(n, (c + 1) * chunk)); chunk = sumsq_chunk(n), never the grid.  The
// squares are formed and summed in fp64: the square of a finite float (< 1.2e77) cannot overflow a double, so the sum is
// non-finite exactly when an input is, and the fixed lane -> wave -> block order makes the partial a function of the
// data alone.
static long sumsq_chunk(long n) {
  long chunk = 16384;
  while ((n + chunk - 1) / chunk > 8192) chunk <<= 1;
  return chunk;
}

__device__ __forceinline__ double block_sum_f64(double a, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = a;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void grad_sumsq_partial_kernel(const float* __restrict__ g, long n, long chunk,
                                                                 double* __restrict__ ws) {
  __shared__ double red[4];
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = c0 + chunk < n ? c0 + chunk : n;
  const long v0 = c0 >> 2, v1 = c1 >> 2;  // (chunk % 4 == 0: c0 is a multiple of 4)
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  long i = v0 + threadIdx.x;
  for (; i + 768 < v1; i += 1024) {  // four 16-byte loads in flight per lane
    const f32x4 x0 = *(const f32x4*)(g + 4 * i), x1 = *(const f32x4*)(g + 4 * (i + 256));
    const f32x4 x2 = *(const f32x4*)(g + 4 * (i + 512)), x3 = *(const f32x4*)(g + 4 * (i + 768));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0 += (double)x0[e] * (double)x0[e];
      a1 += (double)x1[e] * (double)x1[e];
      a2 += (double)x2[e] * (double)x2[e];
      a3 += (double)x3[e] * (double)x3[e];
    }
  }
  for (; i < v1; i += 256) {
    const f32x4 x0 = *(const f32x4*)(g + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) a0 += (double)x0[e] * (double)x0[e];
  }
  const long t = (v1 << 2) + threadIdx.x;  // scalar tail (n % 4, last chunk only)
  if (t < c1) a1 += (double)g[t] * (double)g[t];
  const double s = block_sum_f64((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// Stage 2: ONE workgroup; thread t adds its contiguous run of partials in index order, the 256 thread sums go through
// the same fixed tree.  No atomics anywhere: store pass + ordered sum pass.
__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(const double* __restrict__ ws, int chunks, float grad_scale,
                                                               mdt_guard_state* __restrict__ gs, int accumulate) {
  __shared__ double red[4];
  const int per = (chunks + 255) / 256;
  const int lo = threadIdx.x * per, hi = lo + per < chunks ? lo + per : chunks;
  double a = 0.;
  for (int j = lo; j < hi; ++j) a += ws[j];
  const double s = block_sum_f64(a, red);
  if (threadIdx.x == 0) {
    const double bad = isfinite(s) ? 0. : 1.;
    gs->sumsq = accumulate ? gs->sumsq + s : s;
    gs->nonfinite = accumulate ? gs->nonfinite + bad : bad;
    gs->grad_scale = grad_scale;
  }
}

__global__ void guard_decide_kernel(mdt_guard_state* __restrict__ gs, float max_norm, int skip_nonfinite, double beta1,
                                    double beta2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double ss = gs->sumsq;
  const bool bad = gs->nonfinite != 0. || !isfinite(ss);  // (an all-reduced flag is a count; a NaN sum flags itself)
  const float norm = (float)((double)gs->grad_scale * sqrt(ss));
  const int skip = skip_nonfinite && bad;
  float coef = 1.f;
  if (max_norm > 0.f) {  // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
    const float c = max_norm / (norm + 1e-6f);
    coef = c < 1.f ? c : 1.f;
  }
  gs->norm = norm;
  gs->coef = coef;
  gs->skip = skip;
  if (skip) {
    gs->skipped += 1;
  } else {
    const long long t = gs->applied + 1;
    gs->applied = t;
    gs->inv_bc1 = 1.f / (float)(1. - pow(beta1, (double)t));
    gs->inv_sqrt_bc2 = 1.f / sqrtf((float)(1. - pow(beta2, (double)t)));
  }
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float decay) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) ema[i] = decay * ema[i] + (1.f - decay) * p[i];
}

// table entry: src_off, dst_off, rows, cols, tile_start   (tiles are 64x64, row-major over ceil(rows/64) x ceil(cols/64))
__global__ __launch_bounds__(256) void transpose_batched_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                                const int64_t* __restrict__ table, int n_entries) {
  __shared__ bf16 tile[64][66];
  const int tid = blockIdx.x;
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {  // last entry with tile_start <= tid
    int mid = (lo + hi + 1) >> 1;
    if (table[mid * 5 + 4] <= tid) lo = mid; else hi = mid - 1;
  }
  const int64_t* e = table + lo * 5;
  const long so = e[0], dof = e[1];
  const int rows = (int)e[2], cols = (int)e[3];
  const int local = tid - (int)e[4];
  const int tc = (cols + 63) / 64;
  const int tr_ = local / tc, tc_ = local - tr_ * tc;
  const int r0 = tr_ * 64, c0 = tc_ * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if (r0 + 64 <= rows && c0 + 64 <= cols && ((rows | cols) & 7) == 0 && ((so | dof) & 7) == 0) {
    // full tile, 16-byte accesses on both sides (round 6: the 2-byte form below moved the 2.8 GB of a step's K-major
    // shadows at 2.4 TB/s; every matrix of every shipped model takes this path).  Thread (rr, cq): row rr + 32 pass,
    // columns 8 cq .. 8 cq + 7 -> LDS; then output row (= source column) oc + 32 pass, source rows 8 rq .. 8 rq + 7.
    const int rr = threadIdx.x >> 3, cq = threadIdx.x & 7;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int r = rr + 32 * ps;
      const bf16x8 v = *(const bf16x8*)(src + so + (long)(r0 + r) * cols + c0 + 8 * cq);
#pragma unroll
      for (int e = 0; e < 8; ++e) tile[r][8 * cq + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int oc = rr + 32 * ps;  // output row = source column
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tile[8 * cq + e][oc];
      *(bf16x8*)(dst + dof + (long)(c0 + oc) * rows + r0 + 8 * cq) = v;
    }
    return;
  }
  for (int r = ty; r < 64; r += 4)
    if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = src[so + (long)(r0 + r) * cols + c0 + tx];
  __syncthreads();
  for (int c = ty; c < 64; c += 4)
    if (c0 + c < cols && r0 + tx < rows) dst[dof + (long)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

static int adamw_blocks(long n4) {
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (blocks < 1) blocks = 1;
  return blocks;
}

extern "C" int mdt_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, mdt_bf16* w16, long n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                  float bc2, float ema_decay, float grad_scale, mdt_stream_t stream) {
  MDT_REQUIRE(p && g && m && v, "adamw: null pointer");
  MDT_REQUIRE(n > 0 && bc1 > 0.f && bc2 > 0.f, "adamw: bad arguments");
  MDT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)w16 & 7) == 0,
              "adamw: arenas must be 16-byte aligned");
  long n4 = n >> 2;
  hipLaunchKernelGGL(adamw_ema_kernel<false>, dim3(adamw_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                     (bf16*)w16, n4, n, lr, beta1, beta2, eps, weight_decay, 1.f / bc1, 1.f / sqrtf(bc2), ema_decay, grad_scale,
                     (const mdt_guard_state*)nullptr, 0);
  return mdt_check_launch("adamw_ema_step");
}

extern "C" int mdt_adamw_ema_step_guarded(float* p, const float* g, float* m, float* v, float* ema, mdt_bf16* w16, long n,
                                          float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                          float bc2, float ema_decay, float grad_scale, const mdt_guard_state* state,
                                          int device_bc, mdt_stream_t stream) {
  MDT_REQUIRE(p && g && m && v, "adamw_guarded: null pointer");
  MDT_REQUIRE(state, "adamw_guarded: null guard state");
  MDT_REQUIRE(n > 0 && (device_bc || (bc1 > 0.f && bc2 > 0.f)), "adamw_guarded: bad arguments");
  MDT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)w16 & 7) == 0,
              "adamw_guarded: arenas must be 16-byte aligned");
  MDT_REQUIRE(((uintptr_t)state & 15) == 0, "adamw_guarded: the guard state must be 16-byte aligned");
  long n4 = n >> 2;
  const float ib1 = device_bc ? 1.f : 1.f / bc1, ib2 = device_bc ? 1.f : 1.f / sqrtf(bc2);
  hipLaunchKernelGGL(adamw_ema_kernel<true>, dim3(adamw_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                     (bf16*)w16, n4, n, lr, beta1, beta2, eps, weight_decay, ib1, ib2, ema_decay, grad_scale, state, device_bc);
  return mdt_check_launch("adamw_ema_step_guarded");
}

extern "C" long mdt_grad_sumsq_chunk(long n) { return n > 0 ? sumsq_chunk(n) : 0; }

extern "C" long mdt_grad_sumsq_ws_floats(long n) {
  if (n <= 0) return 0;
  const long chunk = sumsq_chunk(n);
  return 2 * ((n + chunk - 1) / chunk);  // one fp64 partial per chunk
}

extern "C" int mdt_grad_sumsq(const float* g, long n, float grad_scale, float* ws, long ws_floats, mdt_guard_state* state,
                              int accumulate, mdt_stream_t stream) {
  MDT_REQUIRE(g && ws && state, "grad_sumsq: null pointer");
  MDT_REQUIRE(n > 0, "grad_sumsq: n must be positive");
  MDT_REQUIRE((((uintptr_t)g | (uintptr_t)ws | (uintptr_t)state) & 15) == 0,
              "grad_sumsq: gradient range, workspace and guard state must be 16-byte aligned");
  MDT_REQUIRE(ws_floats >= mdt_grad_sumsq_ws_floats(n), "grad_sumsq: workspace smaller than mdt_grad_sumsq_ws_floats(n)");
  const long chunk = sumsq_chunk(n);
  const int chunks = (int)((n + chunk - 1) / chunk);
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(chunks), dim3(256), 0, (hipStream_t)stream, g, n, chunk, (double*)ws);
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, chunks, grad_scale,
                     state, accumulate);
  return mdt_check_launch("grad_sumsq");
}

extern "C" int mdt_guard_decide(mdt_guard_state* state, float max_norm, int skip_nonfinite, double beta1, double beta2,
                                mdt_stream_t stream) {
  MDT_REQUIRE(state, "guard_decide: null guard state");
  MDT_REQUIRE(((uintptr_t)state & 15) == 0, "guard_decide: the guard state must be 16-byte aligned");
  MDT_REQUIRE(max_norm >= 0.f && max_norm <= 3.4e38f, "guard_decide: max_norm must be finite and >= 0 (0 = no clipping)");
  MDT_REQUIRE(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., "guard_decide: betas must lie in [0, 1)");
  hipLaunchKernelGGL(guard_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, max_norm, skip_nonfinite, beta1, beta2);
  return mdt_check_launch("guard_decide");
}

extern "C" int mdt_ema_update(float* ema, const float* p, long n, float decay, mdt_stream_t stream) {
  MDT_REQUIRE(ema && p && n > 0, "ema_update: bad arguments");
  int blocks = (int)((n + 255) / 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(ema_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ema, p, n, decay);
  return mdt_check_launch("ema_update");
}

extern "C" int mdt_transpose_bf16_batched(const mdt_bf16* src, mdt_bf16* dst, const int64_t* table, int n_entries,
                                          int total_tiles, mdt_stream_t stream) {
  MDT_REQUIRE(src && dst && table && n_entries > 0 && total_tiles > 0, "transpose: bad arguments");
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, (const bf16*)src,
                     (bf16*)dst, table, n_entries);
  return mdt_check_launch("transpose_batched");
}
