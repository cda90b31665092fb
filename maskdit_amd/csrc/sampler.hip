// EDM Heun sampler state updates (fp64 state, fp32 network I/O) as fused elementwise kernels
// that read their per-step scalars from a device-side schedule, so that ONE captured hipGraph
// (2 network evaluations + these kernels) replays for every step.
//
// Reference: edm_sampler (sample.py:30-66) with S_churn = 0 (gamma = 0 => x_hat = x_cur,
// t_hat = t_cur); classifier-free guidance combine of DiT.forward_with_cfg
// (models/maskdit.py:580-583) and the EDMPrecond output (models/maskdit.py:764-772).
#include "common.h"
#include "../../include/maskdit_hip.h"

__device__ __forceinline__ void precond_f(float sigma, float sd, float& c_skip, float& c_out, float& c_in) {
  float s2 = sigma * sigma, d2 = sd * sd;
  c_skip = d2 / (s2 + d2);
  c_out = sigma * sd / sqrtf(s2 + d2);
  c_in = 1.f / sqrtf(d2 + s2);
}

// xin[dup copies] = c_in(t) * float(x);  sigma_out[b] = t   (which: 0 -> t_cur, 1 -> t_next)
__global__ void sampler_prep_kernel(const double* __restrict__ x, const double* __restrict__ t_steps,
                                    const int32_t* __restrict__ step_idx, int which, float* __restrict__ xin,
                                    float* __restrict__ sigma_out, int B, int chw, int dup, float sd) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * chw;
  const float sigma = (float)t_steps[*step_idx + which];
  if (idx < (long)B * dup) sigma_out[idx] = sigma;
  if (idx >= n) return;
  float cs, co, ci;
  precond_f(sigma, sd, cs, co, ci);
  float v = ci * (float)x[idx];
  xin[idx] = v;
  if (dup > 1) xin[n + idx] = v;
}

__device__ __forceinline__ double denoise(const double xh, const float* F, long idx, long n, float sigma, float sd,
                                          float cfg_scale, int use_cfg) {
  float f = F[idx];
  if (use_cfg) {
    float fu = F[n + idx];
    f = fu + cfg_scale * (f - fu);
  }
  float cs, co, ci;
  precond_f(sigma, sd, cs, co, ci);
  // the network sees x_hat.float(); D = c_skip * x + c_out * F in fp32, then .to(float64)
  return (double)(cs * (float)xh + co * f);
}

__global__ void sampler_euler_kernel(const double* __restrict__ x_hat, const float* __restrict__ F,
                                     const double* __restrict__ t_steps, const int32_t* __restrict__ step_idx,
                                     float cfg_scale, int use_cfg, double* __restrict__ x_next,
                                     double* __restrict__ d_cur, long n, float sd) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int i = *step_idx;
  const double t_hat = t_steps[i], t_next = t_steps[i + 1];
  const double xh = x_hat[idx];
  const double den = denoise(xh, F, idx, n, (float)t_hat, sd, cfg_scale, use_cfg);
  const double d = (xh - den) / t_hat;
  d_cur[idx] = d;
  x_next[idx] = xh + (t_next - t_hat) * d;
}

__global__ void sampler_heun_kernel(const double* __restrict__ x_hat, double* __restrict__ x_next,
                                    const float* __restrict__ F, const double* __restrict__ d_cur,
                                    const double* __restrict__ t_steps, const int32_t* __restrict__ step_idx,
                                    float cfg_scale, int use_cfg, long n, float sd) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int i = *step_idx;
  const double t_hat = t_steps[i], t_next = t_steps[i + 1];
  const double xn = x_next[idx];
  const double den = denoise(xn, F, idx, n, (float)t_next, sd, cfg_scale, use_cfg);
  const double d_prime = (xn - den) / t_next;
  x_next[idx] = x_hat[idx] + (t_next - t_hat) * (0.5 * d_cur[idx] + 0.5 * d_prime);
}

__global__ void sampler_advance_kernel(int32_t* step_idx) { *step_idx += 1; }

extern "C" int mdt_sampler_prep(const double* x, const double* t_steps, const int32_t* step_idx, int which, float* xin,
                                float* sigma_out, int B, int chw, int dup, float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x && t_steps && step_idx && xin && sigma_out, "sampler_prep: null pointer");
  MDT_REQUIRE(dup == 1 || dup == 2, "sampler_prep: dup must be 1 or 2");
  long n = (long)B * chw;
  hipLaunchKernelGGL(sampler_prep_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, t_steps, step_idx,
                     which, xin, sigma_out, B, chw, dup, sigma_data);
  return mdt_check_launch("sampler_prep");
}

extern "C" int mdt_sampler_euler(const double* x_hat, const float* F, const double* t_steps, const int32_t* step_idx,
                                 float cfg_scale, int use_cfg, double* x_next, double* d_cur, int B, int chw,
                                 float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x_hat && F && t_steps && step_idx && x_next && d_cur, "sampler_euler: null pointer");
  long n = (long)B * chw;
  hipLaunchKernelGGL(sampler_euler_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_hat, F, t_steps,
                     step_idx, cfg_scale, use_cfg, x_next, d_cur, n, sigma_data);
  return mdt_check_launch("sampler_euler");
}

extern "C" int mdt_sampler_heun(const double* x_hat, double* x_next, const float* F, const double* d_cur,
                                const double* t_steps, const int32_t* step_idx, float cfg_scale, int use_cfg, int B,
                                int chw, float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x_hat && x_next && F && d_cur && t_steps && step_idx, "sampler_heun: null pointer");
  long n = (long)B * chw;
  hipLaunchKernelGGL(sampler_heun_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_hat, x_next, F, d_cur,
                     t_steps, step_idx, cfg_scale, use_cfg, n, sigma_data);
  return mdt_check_launch("sampler_heun");
}

extern "C" int mdt_sampler_advance(int32_t* step_idx, mdt_stream_t stream) {
  MDT_REQUIRE(step_idx, "sampler_advance: null pointer");
  hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_idx);
  return mdt_check_launch("sampler_advance");
}

// out[B] = F_uncond + s * (F_cond - F_uncond) with F = [cond; uncond] (models/maskdit.py:580-583)
__global__ void cfg_combine_kernel(const float* __restrict__ F, float s, float* __restrict__ out, long n) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  float fu = F[n + idx];
  out[idx] = fu + s * (F[idx] - fu);
}

extern "C" int mdt_cfg_combine(const float* F, float cfg_scale, float* out, long n, mdt_stream_t stream) {
  MDT_REQUIRE(F && out && n > 0, "cfg_combine: bad arguments");
  hipLaunchKernelGGL(cfg_combine_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, F, cfg_scale, out, n);
  return mdt_check_launch("cfg_combine");
}

// ---------------------------------------------------------------------------------------------------------------------
// ablation_sampler (sample.py:73-188): the generalized step reads every per-step scalar from row *step_idx of an fp64
// table (MDT_ABL_* columns, include/maskdit_hip.h), so one captured graph serves every step of every discretization,
// schedule and scaling.  FP contraction is off: each fp64 / fp32 operation rounds once, as the reference's torch ops do.

__device__ __forceinline__ float ablation_denoise(float xi, const float* F, long idx, long n, float sigma, float sd,
                                                  float cfg_scale, int use_cfg) {
#pragma clang fp contract(off)
  float f = F[idx];
  if (use_cfg) {
    float fu = F[n + idx];
    f = fu + cfg_scale * (f - fu);
  }
  float cs, co, ci;
  precond_f(sigma, sd, cs, co, ci);
  return cs * xi + co * f;  // D = c_skip * x_in + c_out * F, x_in = float(x) / s (models/maskdit.py:771)
}

__global__ void ablation_prep_kernel(const double* __restrict__ x, const double* __restrict__ noise,
                                     const double* __restrict__ table, const int32_t* __restrict__ step_idx, int which,
                                     double* __restrict__ x_hat, float* __restrict__ xin, float* __restrict__ sigma_out,
                                     int B, int chw, int dup, float sd) {
#pragma clang fp contract(off)
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * chw;
  const double* row = table + (long)*step_idx * MDT_ABL_NCOL;
  const float sigma = (float)row[which ? MDT_ABL_SIG2 : MDT_ABL_SIG];
  const float s = (float)row[which ? MDT_ABL_S2 : MDT_ABL_S];
  if (idx < (long)B * dup) sigma_out[idx] = sigma;
  if (idx >= n) return;
  double v = x[idx];
  if (!which) {
    v = row[MDT_ABL_A] * v + row[MDT_ABL_C] * noise[idx];  // sample.py:167
    x_hat[idx] = v;
  }
  float cs, co, ci;
  precond_f(sigma, sd, cs, co, ci);
  const float xi = ci * ((float)v / s);  // sample.py:172 x_hat.float() / s(t_hat), then c_in (models/maskdit.py:769)
  xin[idx] = xi;
  if (dup > 1) xin[n + idx] = xi;
}

__global__ void ablation_slope1_kernel(const double* __restrict__ x_hat, const float* __restrict__ F,
                                       const double* __restrict__ table, const int32_t* __restrict__ step_idx,
                                       float cfg_scale, int use_cfg, double* __restrict__ d_cur, double* __restrict__ x,
                                       long n, float sd) {
#pragma clang fp contract(off)
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const double* row = table + (long)*step_idx * MDT_ABL_NCOL;
  const double xh = x_hat[idx];
  const float xi = (float)xh / (float)row[MDT_ABL_S];
  const double den = (double)ablation_denoise(xi, F, idx, n, (float)row[MDT_ABL_SIG], sd, cfg_scale, use_cfg);
  const double d = row[MDT_ABL_P] * xh - row[MDT_ABL_Q] * den;  // sample.py:173-174
  d_cur[idx] = d;
  // sample.py:175 x_prime for the second evaluation, or sample.py:180 x_next
  x[idx] = xh + (row[MDT_ABL_SECOND] != 0.0 ? row[MDT_ABL_AH] : row[MDT_ABL_H]) * d;
}

__global__ void ablation_slope2_kernel(const double* __restrict__ x_hat, double* __restrict__ x,
                                       const float* __restrict__ F, const double* __restrict__ d_cur,
                                       const double* __restrict__ table, const int32_t* __restrict__ step_idx,
                                       float cfg_scale, int use_cfg, long n, float sd) {
#pragma clang fp contract(off)
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const double* row = table + (long)*step_idx * MDT_ABL_NCOL;
  const double xp = x[idx];
  const float xi = (float)xp / (float)row[MDT_ABL_S2];
  const double den = (double)ablation_denoise(xi, F, idx, n, (float)row[MDT_ABL_SIG2], sd, cfg_scale, use_cfg);
  const double dp = row[MDT_ABL_P2] * xp - row[MDT_ABL_Q2] * den;  // sample.py:184-185
  x[idx] = x_hat[idx] + row[MDT_ABL_H] * (row[MDT_ABL_W1] * d_cur[idx] + row[MDT_ABL_W2] * dp);  // sample.py:186
}

extern "C" int mdt_ablation_prep(const double* x, const double* noise, const double* table, const int32_t* step_idx,
                                 int which, double* x_hat, float* xin, float* sigma_out, int B, int chw, int dup,
                                 float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x && table && step_idx && xin && sigma_out, "ablation_prep: null pointer");
  MDT_REQUIRE(which == 0 || which == 1, "ablation_prep: which must be 0 or 1");
  MDT_REQUIRE(which == 1 || (noise && x_hat), "ablation_prep: which = 0 needs noise and x_hat");
  MDT_REQUIRE(dup == 1 || dup == 2, "ablation_prep: dup must be 1 or 2");
  MDT_REQUIRE(B > 0 && chw >= dup, "ablation_prep: bad shape");
  long n = (long)B * chw;
  hipLaunchKernelGGL(ablation_prep_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, noise, table,
                     step_idx, which, x_hat, xin, sigma_out, B, chw, dup, sigma_data);
  return mdt_check_launch("ablation_prep");
}

extern "C" int mdt_ablation_slope1(const double* x_hat, const float* F, const double* table, const int32_t* step_idx,
                                   float cfg_scale, int use_cfg, double* d_cur, double* x, int B, int chw,
                                   float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x_hat && F && table && step_idx && d_cur && x, "ablation_slope1: null pointer");
  MDT_REQUIRE(B > 0 && chw > 0, "ablation_slope1: bad shape");
  long n = (long)B * chw;
  hipLaunchKernelGGL(ablation_slope1_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_hat, F, table,
                     step_idx, cfg_scale, use_cfg, d_cur, x, n, sigma_data);
  return mdt_check_launch("ablation_slope1");
}

extern "C" int mdt_ablation_slope2(const double* x_hat, double* x, const float* F, const double* d_cur,
                                   const double* table, const int32_t* step_idx, float cfg_scale, int use_cfg, int B,
                                   int chw, float sigma_data, mdt_stream_t stream) {
  MDT_REQUIRE(x_hat && x && F && d_cur && table && step_idx, "ablation_slope2: null pointer");
  MDT_REQUIRE(B > 0 && chw > 0, "ablation_slope2: bad shape");
  long n = (long)B * chw;
  hipLaunchKernelGGL(ablation_slope2_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_hat, x, F, d_cur,
                     table, step_idx, cfg_scale, use_cfg, n, sigma_data);
  return mdt_check_launch("ablation_slope2");
}
