// Token-boundary kernels for patch vectors of 64 and 256 elements (C = 4, patch 4 and 8): csrc/patch.hip.  The six public
// entries (mdt_patch_embed_fwd / bwd, mdt_final_fwd / bwd, mdt_edm_loss_fwd / bwd) dispatch here when C * p * p > 16.
#pragma once
#include "common.h"

static inline bool mdt_wide_patch(int C, int p) { return C * p * p == 64 || C * p * p == 256; }

int mdt_wide_patch_embed_fwd(const float* x, const float* in_scale, const float* W, const float* bias, const float* pos,
                             const int32_t* ids, int ids_ld, float* out, int B, int C, int R, int p, int L, int D,
                             hipStream_t stream);
int mdt_wide_patch_embed_bwd(const float* x, const float* in_scale, const float* dout, const int32_t* ids, int ids_ld,
                             float* dW, float* dbias, int B, int C, int R, int p, int L, int D, hipStream_t stream);
int mdt_wide_final_fwd(const float* x, const float* shift, const float* scale, int mod_ld, const float* W, const float* bias,
                       float* F, float* stats, int B, int T, int Dd, int C, int p, hipStream_t stream);
int mdt_wide_final_bwd(const float* dF, const float* x, const float* stats, const float* shift, const float* scale, int mod_ld,
                       const float* W, float* dx, float* dW, float* dbias, float* dshift, float* dscale, int dmod_ld, int B,
                       int T, int Dd, int C, int p, hipStream_t stream);
int mdt_wide_edm_loss_fwd(const float* F, const float* yn, const float* y, const float* coef, const float* mask,
                          float mae_coef, float* D, float* loss, int B, int C, int R, int p, hipStream_t stream);
int mdt_wide_edm_loss_bwd(const float* dloss, const float* D, const float* yn, const float* y, const float* coef,
                          const float* mask, float mae_coef, float* dF, int B, int C, int R, int p, hipStream_t stream);
