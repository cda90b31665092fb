// The fp32-FAITHFUL inference path (VERDICT r5 missing #3 / next #4): the reference's sampler runs its network in fp32
// (sample.py:56 `net(x_hat.float(), ...)`, no autocast in generate.py) and `train.py --no_amp` does the same for training;
// rounds 1-5 only had the bf16-operand kernels, so BASELINE configs[4] was measured at narrower arithmetic than the
// reference's own.  Everything here computes in EXACT fp32: weights are read straight from the fp32 master arena (no
// shadow), activations stay fp32 in HBM, and the GEMMs use the fp32-input matrix instruction
// v_mfma_f32_32x32x2_f32 (64 FLOP/clk/SIMD = the fp32 vector rate, 157 TFLOP/s per chip: 1/16 of the bf16 rate; there is
// no TF32 / xf32 on gfx950).  What torch's fp32 nn.Linear / SDPA / LayerNorm do on this chip is the same arithmetic in
// another summation order, so the two agree to fp32 rounding (tests: 1e-5 of the output range after 99 evaluations).
//
//   mdt_gemm_f32        C = A * B^T (+ bias) with fp32 epilogues (none / GELU-tanh / SiLU / res + gate * y), batched over
//                       (sample, head) with independent strides -- also serves attention (scores = q k^T, out = p v)
//   mdt_softmax_rows_f32  in-place row softmax of the scores (timm Attention: softmax(q k^T * hd^-0.5))
//   mdt_ln_modulate_f32 LayerNorm(eps 1e-6, no affine) * (1 + scale) + shift -> fp32      (models/maskdit.py:19-20,177)
//   mdt_timestep_embed_f32, mdt_silu_f32, mdt_add_rows_f32   conditioning path / position embedding glue
//
// Reference: DiTBlock.forward (models/maskdit.py:188-192), timm Attention / Mlp (call sites :178,182),
// TimestepEmbedder (:41-60), LabelEmbedder (:75), DecoderLayer (:195-213), decoder_pos_embed add (:545).
//
// GEMM design.  f32 MFMA is 16x slower than the bf16 one while the operand bytes only double, so the kernel is
// matrix-pipe-bound by a wide margin with a plain structure: 128 x (32 NB WN) tile, 4 waves, K-tile of 32 floats staged
// through registers into a double-buffered LDS image (one workgroup barrier per K-tile; hipcc counts the waits -- nothing
// hand-counted here).  Per K-tile a wave issues 16 MB NB MFMAs (64 clocks each) against 4 (MB + NB) ds_read_b128.
// The contraction index is PERMUTED inside a K-tile: lane (r, kh) of a fragment reads four consecutive k of its row with
// one 16-byte LDS read and feeds them to four successive MFMAs -- A and B use the same permutation, so the sum is over
// all 32 k; a 16-byte-chunk XOR swizzle (chunk ^ row & 7) spreads the rows of a fragment over the banks.
#include "common.h"
#include "../../include/maskdit_hip.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace f32p {

struct Params {
  const float* A; long lda;
  const float* B; long ldb;
  int M, N, K;
  const float* bias;
  int epi;
  float* out; long ldo;
  const float* res; long ldres;
  const float* gate; long gate_ld; int rps;
  int heads;
  long a_sb, a_sh, b_sb, b_sh, o_sb, o_sh;
  int vec_ok;  // 16-byte epilogue accesses are legal: out / res / gate / bias pitches and bases are multiples of 4 floats
  int dbg;  // experiments build only (MDT_F32_ABLATE: 1 = no global loads / LDS stores in the K loop, 2 = no barrier, 4 = no fragment reads; garbage results)
};

// exact-form activations (torch: F.gelu(approximate='tanh'), F.silu) -- the bf16 path's exp2 / rcp forms are 1-ulp
// approximations rounded to bf16 afterwards; here the result IS the fp32 output
__device__ __forceinline__ float gelu_tanh_f32(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return 0.5f * x * (1.f + tanhf(u));
}
__device__ __forceinline__ float silu_f32(float x) { return x / (1.f + expf(-x)); }

// ---- epilogue shared by the GEMM forms: the lane's output row m = block row lane & 31; register quad q4 of block jj =
// columns nq .. nq + 3 (the accumulator blocks are the TRANSPOSED output blocks: see fmma)
template <int MB, int NB>
__device__ __forceinline__ void f32_epilogue(const Params& p, f32x16 (&acc)[MB][NB], int m0, int n0, int wm, int wn, int r, int kh,
                                             float* __restrict__ out) {
  const int epi = p.epi;
  const bool vec = p.vec_ok;  // 16-byte accesses legal (pitches / bases multiples of 4 floats; checked by the host entry)
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int m = m0 + (wm * MB + i) * 32 + r;
    if (m >= p.M) continue;
    float* orow = out + (long)m * p.ldo;
    const float* rrow = epi == MDT_F32EPI_GATE_RES ? p.res + (long)m * p.ldres : nullptr;
    const float* grow = (epi == MDT_F32EPI_GATE_RES && p.gate) ? p.gate + (long)(m / p.rps) * p.gate_ld : nullptr;
#pragma unroll
    for (int jj = 0; jj < NB; ++jj) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int nq = n0 + (wn * NB + jj) * 32 + 8 * q4 + 4 * kh;
        if (nq >= p.N) continue;
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = acc[i][jj][4 * q4 + e];
        if (vec && nq + 4 <= p.N) {
          if (p.bias) {
            const f32x4 b4 = *(const f32x4*)(p.bias + nq);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] += b4[e];
          }
          if (epi == MDT_F32EPI_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = gelu_tanh_f32(y[e]);
          } else if (epi == MDT_F32EPI_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = silu_f32(y[e]);
          } else if (epi == MDT_F32EPI_GATE_RES) {
            const f32x4 r4 = *(const f32x4*)(rrow + nq);
            f32x4 g4 = (f32x4){1.f, 1.f, 1.f, 1.f};
            if (grow) g4 = *(const f32x4*)(grow + nq);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = r4[e] + g4[e] * y[e];
          }
          *(f32x4*)(orow + nq) = (f32x4){y[0], y[1], y[2], y[3]};
        } else {  // ragged / unaligned: element by element
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int n = nq + e;
            if (n >= p.N) continue;
            float v = y[e] + (p.bias ? p.bias[n] : 0.f);
            if (epi == MDT_F32EPI_GELU) v = gelu_tanh_f32(v);
            else if (epi == MDT_F32EPI_SILU) v = silu_f32(v);
            else if (epi == MDT_F32EPI_GATE_RES) v = rrow[n] + (grow ? grow[n] : 1.f) * v;
            orow[n] = v;
          }
        }
      }
    }
  }
}

// BKT = floats per K-tile (32 or 16): 128-byte or 64-byte LDS rows of BKT / 4 16-byte chunks, chunk c of row r stored at
// chunk c ^ (r & (BKT / 4 - 1)).
template <int WM, int WN, int MB, int NB, int BKT, bool BKM>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const Params p, const int tiles_m, const int tiles_n) {
  constexpr int BM = WM * MB * 32, BN = WN * NB * 32;
  constexpr int CPRW = BKT / 4, NG = BKT / 8;        // 16-byte chunks per row; step groups (8 k each) per K-tile
  static_assert(WM * WN == 4, "four waves");
  static_assert(BKT == 16 || BKT == 32, "K-tile depth");
  constexpr int A_CH = BM * CPRW / 256;              // 16-byte chunks per thread and K-tile
  constexpr int B_CH = BN * CPRW / 256;
  static_assert(A_CH >= 1 && B_CH >= 1, "tile too small for 256 threads");
  __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * BKT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  // XCD-contiguous tile ids (block b runs on XCD b % 8)
  const int nt = tiles_m * tiles_n;
  int t = blockIdx.x;
  {
    const int q = nt >> 3, r = nt & 7, x = t & 7, i = t >> 3;
    t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  // grouped order: 8 row panels x 1 column panel, next column panel, ... -- the workgroups an XCD holds at a time cover
  // ~8 x 8 panels whose current K-tiles live in its L2 while they advance together (row-major order: L2 hit rate 0.49,
  // this order 0.80 -- profiles/r6_f32_pmc.txt; by itself it did not change the launch time, see the K-loop note below).
  constexpr int GM = 8;
  const int per_group = GM * tiles_n, grp = t / per_group, first_m = grp * GM;
  const int gm = min(tiles_m - first_m, GM), in_g = t - grp * per_group;
  const int tm = first_m + in_g % gm, tn = in_g / gm;
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.y, zb = z / p.heads, zh = z - zb * p.heads;
  const float* __restrict__ A = p.A + zb * p.a_sb + zh * p.a_sh;
  const float* __restrict__ Bm = p.B + zb * p.b_sb + zh * p.b_sh;
  float* __restrict__ out = p.out + zb * p.o_sb + zh * p.o_sh;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // ---- global -> register staging, TWO K-tiles ahead (two register sets): a load issued at the top of iteration kt is
  // stored to LDS at the end of iteration kt + 1, so no wave ever parks on vmcnt for a load younger than a whole K-tile
  // of MFMAs.  Row pointers / row masks are loop-invariant; the K bound only matters in the last K-tile.
  f32x4 ga[2][A_CH], gb[2][B_CH];
  const float* pa[A_CH];
  const float* pb[B_CH];
  bool oka[A_CH], okb[B_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int q = tid + 256 * i, row = q / CPRW, c = q % CPRW;
    oka[i] = (m0 + row) < p.M;
    pa[i] = A + (long)min(m0 + row, p.M - 1) * p.lda + 4 * c;
  }
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    const int q = tid + 256 * i;
    if (!BKM) {
      const int row = q / CPRW, c = q % CPRW;
      okb[i] = (n0 + row) < p.N;
      pb[i] = Bm + (long)min(n0 + row, p.N - 1) * p.ldb + 4 * c;
    } else {  // B is [K][N]: a K-tile is BKT rows of BN floats; chunk q = row kr = q / (BN / 4), columns 4 (q % (BN / 4))
      const int kr = q / (BN / 4), c = q % (BN / 4);
      okb[i] = (n0 + 4 * c) < p.N;
      pb[i] = Bm + (long)kr * p.ldb + min(n0 + 4 * c, p.N - 4);
    }
  }
  const bool k_ragged = (p.K % BKT) != 0;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto gload = [&](auto set_c, int k0) {
    constexpr int set = decltype(set_c)::value;
    if (!k_ragged || k0 + BKT <= p.K) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const f32x4 v = *(const f32x4*)(pa[i] + k0);
        ga[set][i] = oka[i] ? v : zero4;
      }
#pragma unroll
      for (int i = 0; i < B_CH; ++i) {
        const f32x4 v = *(const f32x4*)(BKM ? pb[i] + (long)k0 * p.ldb : pb[i] + k0);
        gb[set][i] = okb[i] ? v : zero4;
      }
    } else {  // last, partial K-tile: chunks at or beyond K read as zeros (addresses stay inside the operands)
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int c4 = 4 * ((tid + 256 * i) % CPRW);
        const f32x4 v = *(const f32x4*)(pa[i] + min(k0, p.K - 4 - c4));
        ga[set][i] = (oka[i] && k0 + c4 < p.K) ? v : zero4;
      }
#pragma unroll
      for (int i = 0; i < B_CH; ++i) {
        if (!BKM) {
          const int c4 = 4 * ((tid + 256 * i) % CPRW);
          const f32x4 v = *(const f32x4*)(pb[i] + min(k0, p.K - 4 - c4));
          gb[set][i] = (okb[i] && k0 + c4 < p.K) ? v : zero4;
        } else {
          const int kr = (tid + 256 * i) / (BN / 4);
          const f32x4 v = *(const f32x4*)(pb[i] + (long)min(k0, p.K - 1 - kr) * p.ldb);
          gb[set][i] = (okb[i] && k0 + kr < p.K) ? v : zero4;
        }
      }
    }
  };
  auto lstore = [&](auto set_c, int buf) {
    constexpr int set = decltype(set_c)::value;
    float* la = lds[buf];
    float* lb = lds[buf] + BM * BKT;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int q = tid + 256 * i, row = q / CPRW, c = q % CPRW;
      *(f32x4*)(la + row * BKT + 4 * (c ^ (row & (CPRW - 1)))) = ga[set][i];
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int q = tid + 256 * i;
      if (!BKM) {
        const int row = q / CPRW, c = q % CPRW;
        *(f32x4*)(lb + row * BKT + 4 * (c ^ (row & (CPRW - 1)))) = gb[set][i];
      } else {
        *(f32x4*)(lb + 4 * q) = gb[set][i];  // [kr][BN], kr = q / (BN / 4)
      }
    }
  };

  const int nk = (p.K + BKT - 1) / BKT;
  const int r = lane & 31, kh = lane >> 5;
  // fragment sets: [set][block] = the four k of step group j (8 k: k = 8 j + 4 kh + e) of a 32-row block
  f32x4 fa[2][MB], fb[2][NB];
  auto fload = [&](int set, int buf, int j) {
    const float* la = lds[buf] + (wm * MB * 32) * BKT;
    const float* lb = lds[buf] + BM * BKT;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const int row = 32 * i + r;  // (tile row & 7) == (row & 7): wm * MB * 32 is a multiple of 8
      fa[set][i] = *(const f32x4*)(la + row * BKT + 4 * ((2 * j + kh) ^ (row & (CPRW - 1))));
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int col = (wn * NB + i) * 32 + r;
      if (!BKM) {
        fb[set][i] = *(const f32x4*)(lb + col * BKT + 4 * ((2 * j + kh) ^ (col & (CPRW - 1))));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) fb[set][i][e] = lb[(8 * j + 4 * kh + e) * BN + col];
      }
    }
  };
  // The MFMA takes the B fragment as its first operand: the accumulator block is the TRANSPOSED output block, i.e. a lane
  // holds, for ONE output row m (= its A row, lane & 31), columns n = 8 (e / 4) + 4 (lane / 32) + e % 4 of the block --
  // four consecutive n per register quad, so the epilogue moves 16 bytes per lane and access.
  auto fmma = [&](int set) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int jj = 0; jj < NB; ++jj)
          acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[set][jj][e], fa[set][i][e], acc[i][jj], 0, 0, 0);
  };
  // K loop, software-pipelined by hand: the fragments of step group j + 1 are read BEFORE the 4 MB NB MFMAs of group j,
  // and the last group of a K-tile runs after the barrier, under the first reads of the next K-tile.  LDS hazards: tile
  // kt + 1 is stored into the buffer tile kt - 1 was read from; those reads were issued before barrier(kt - 1), which
  // waits for them (lgkmcnt(0)).
  // What bounds this kernel (round 6, profiles/r6_f32_*.txt): with every memory instruction of the loop ablated the
  // launch runs at 133-134 TF/s (0.85 of the 157 TF/s peak: prologue / epilogue per 36-K-tile tile); the global loads +
  // LDS stores cost 15 % of the full kernel and the fragment reads 9 %.  NOT the barrier (ablating it: no change), not the
  // LDS read latency (pipelining the reads a whole step group ahead: no change), not L2 misses (hit rate 0.49 -> 0.80 with
  // the grouped tile order: no change), not the operand bytes (256 x 128 x 16 tile, 23 instead of 31 B / kFLOP: no change).
  auto step = [&](auto par_c, int kt) {
    constexpr int par = decltype(par_c)::value;  // = kt & 1: LDS buffer of this K-tile and register set of K-tile kt + 2
    const bool more = kt + 1 < nk;
    if (kt + 2 < nk && !MDT_EXP(p.dbg & 1)) gload(par_c, (kt + 2) * BKT);
#pragma unroll
    for (int g = 0; g + 1 < NG; ++g) {
      if (!MDT_EXP(p.dbg & 4)) fload((g + 1) & 1, par, g + 1);
      __builtin_amdgcn_sched_barrier(0);
      fmma(g & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more && !MDT_EXP(p.dbg & 1)) lstore(std::integral_constant<int, par ^ 1>{}, par ^ 1);
    if (!MDT_EXP(p.dbg & 2)) __syncthreads();
    if (more && !MDT_EXP(p.dbg & 4)) fload(NG & 1, par ^ 1, 0);   // (NG is even: the next tile's group 0 lands in set 0 again)
    __builtin_amdgcn_sched_barrier(0);
    fmma((NG - 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  gload(std::integral_constant<int, 0>{}, 0);
  lstore(std::integral_constant<int, 0>{}, 0);
  if (nk > 1) gload(std::integral_constant<int, 1>{}, BKT);
  __syncthreads();
  fload(0, 0, 0);
  for (int kt = 0; kt < nk; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
  }

  f32_epilogue<MB, NB>(p, acc, m0, n0, wm, wn, r, kh, out);
}

// ------------------------------------------------------------------------------------------------------------------
// The same GEMM with its operand tiles moved by LDS-DMA (global_load_lds, 16 B per lane: 1 KiB of LDS per wave-instruction,
// no staging registers, no ds_write, no per-chunk selects) -- for the Linear layers: 128 x 128 x 32 tile, B = [N][K], K a
// multiple of 32.  The K loop of the register-staged form costs the MFMA waves 8 global loads + 8 LDS stores + ~60 VALU per
// K-tile (15 % of the launch by the ablation of profiles/r6_f32_pmc.txt); here it is 8 DMA instructions.  hipcc's waitcnt pass
// does not know which LDS bytes a DMA in flight writes and would drain vmcnt(0) in front of every LDS read it sees, so the
// fragment reads are inline asm with hand-placed lgkmcnt waits (the idiom of gemm_tn8.hip): reads retire in order, so
// "all but the newest MB + NB reads have landed" is exactly "the previous fragment set is complete".
// Schedule of K-tile kt (buffer b = kt & 1): [DMA of tile kt + 1 into b ^ 1][reads g1][MFMA g0][reads g2][MFMA g1][reads g3]
// [MFMA g2][vmcnt(0) + barrier][reads g0 of tile kt + 1][MFMA g3].  b ^ 1 held tile kt - 1, whose last reads were waited for
// before barrier(kt - 1); the DMA has the whole K-tile to land.  Rows beyond M / N are clamped to the last row: they
// only feed output rows / columns the epilogue never stores.
template <int N> __device__ __forceinline__ void f32_wait_lgkm() {
  __builtin_amdgcn_s_waitcnt(15 | (7 << 4) | ((N & 15) << 8) | (3 << 14));  // vmcnt / expcnt unconstrained
}
__device__ __forceinline__ f32x4 f32_lds_read16(unsigned addr) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

template <int MB, int NB, int BKT, int MINW>
__global__ __launch_bounds__(256, MINW) void gemm_f32_dma_kernel(const Params p, const int tiles_m, const int tiles_n) {
  constexpr int WN = 2, BM = 2 * MB * 32, BN = 2 * NB * 32, NG = BKT / 8;
  constexpr int CPRW = BKT / 4, RP = 64 / CPRW;          // 16-byte chunks per LDS row; rows per 1 KiB piece
  constexpr int A_PC = BM / RP / 4, B_PC = BN / RP / 4;  // pieces per wave and K-tile
  static_assert(BKT == 32 || BKT == 16, "K-tile depth");
  static_assert(A_PC >= 1 && B_PC >= 1 && NG >= 2, "tile too small");
  __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * BKT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int nt = tiles_m * tiles_n;
  int t = blockIdx.x;
  {
    const int q = nt >> 3, r = nt & 7, x = t & 7, i = t >> 3;
    t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  constexpr int GM = 8;
  const int per_group = GM * tiles_n, grp = t / per_group, first_m = grp * GM;
  const int gm = min(tiles_m - first_m, GM), in_g = t - grp * per_group;
  const int tm = first_m + in_g % gm, tn = in_g / gm;
  const int m0 = tm * BM, n0 = tn * BN;
  float* __restrict__ out = p.out;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // DMA sources: piece pc = wave + 4 i covers tile rows RP pc .. RP pc + RP - 1; lane l brings row RP pc + l / CPRW, global
  // chunk (l % CPRW) ^ (row & (CPRW - 1)) -- the XOR swizzle of the register-staged form, applied through the source address
  const int lrow = lane / CPRW, lchunk = (lane % CPRW) ^ (lrow & (CPRW - 1));
  const float* pa[A_PC];
  const float* pb[B_PC];
#pragma unroll
  for (int i = 0; i < A_PC; ++i) pa[i] = p.A + (long)min(m0 + RP * (wave + 4 * i) + lrow, p.M - 1) * p.lda + 4 * lchunk;
#pragma unroll
  for (int i = 0; i < B_PC; ++i) pb[i] = p.B + (long)min(n0 + RP * (wave + 4 * i) + lrow, p.N - 1) * p.ldb + 4 * lchunk;
  auto dma = [&](int buf, int k0) {
    float* la = lds[buf] + wave * 256;          // 1 KiB = 256 floats per piece
    float* lb = lds[buf] + BM * BKT + wave * 256;
#pragma unroll
    for (int i = 0; i < A_PC; ++i) glds16(pa[i] + k0, la + i * 1024);
#pragma unroll
    for (int i = 0; i < B_PC; ++i) glds16(pb[i] + k0, lb + i * 1024);
  };

  const int nk = p.K / BKT;
  const int r = lane & 31, kh = lane >> 5;
  const unsigned lds0 = (unsigned)(size_t)LDS_PTR(&lds[0][0]);
  constexpr unsigned BUF_BYTES = (BM + BN) * BKT * 4;
  unsigned ra[MB], rb[NB];  // byte offsets of this lane's rows inside a buffer
#pragma unroll
  for (int i = 0; i < MB; ++i) ra[i] = (unsigned)(((wm * MB + i) * 32 + r) * BKT) * 4u;
#pragma unroll
  for (int i = 0; i < NB; ++i) rb[i] = (unsigned)((BM + (wn * NB + i) * 32 + r) * BKT) * 4u;
  const int rsw = r & (CPRW - 1);
  f32x4 fa[2][MB], fb[2][NB];
  auto fload = [&](int set, int buf, int j) {
    const unsigned cb = lds0 + buf * BUF_BYTES + 16u * ((2 * j + kh) ^ rsw);
#pragma unroll
    for (int i = 0; i < MB; ++i) fa[set][i] = f32_lds_read16(cb + ra[i]);
#pragma unroll
    for (int i = 0; i < NB; ++i) fb[set][i] = f32_lds_read16(cb + rb[i]);
  };
  auto fmma = [&](int set) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int jj = 0; jj < NB; ++jj)
          acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[set][jj][e], fa[set][i][e], acc[i][jj], 0, 0, 0);
  };
#define F32_FENCE() __builtin_amdgcn_sched_barrier(0)
  dma(0, 0);
  __syncthreads();  // (hipcc waits vmcnt(0) for the release: tile 0 has landed)
  F32_FENCE();
  fload(0, 0, 0);
  F32_FENCE();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {  // every read of the OTHER buffer (tile kt - 1) was waited for before barrier(kt - 1): refill it right away --
      dma(buf ^ 1, (kt + 1) * BKT);  // the DMA then has this whole K-tile of MFMAs to land (issued behind g2: 7 % slower)
      F32_FENCE();
    }
#pragma unroll
    for (int g = 0; g + 1 < NG; ++g) {
      fload((g + 1) & 1, buf, g + 1);
      F32_FENCE();
      f32_wait_lgkm<MB + NB>();  // the set about to be used has landed; the one just requested may be in flight
      F32_FENCE();
      fmma(g & 1);
      F32_FENCE();
    }
    f32_wait_lgkm<0>();  // this wave's reads of `buf` are complete before anyone may overwrite it (after the next barrier)
    F32_FENCE();
    __syncthreads();     // + vmcnt(0): tile kt + 1 is in LDS for every wave
    F32_FENCE();
    if (more) fload(NG & 1, buf ^ 1, 0);
    F32_FENCE();
    fmma((NG - 1) & 1);
    F32_FENCE();
    if (more) f32_wait_lgkm<0>();  // (set 0 of the next tile; the next iteration's first wait counts from a clean queue)
    F32_FENCE();
  }
#undef F32_FENCE
  f32_epilogue<MB, NB>(p, acc, m0, n0, wm, wn, r, kh, out);
}

template <int WM, int WN, int MB, int NB, int BKT>
int launch(const Params& p, bool bkm, int batch, hipStream_t stream) {
  constexpr int BM = WM * MB * 32, BN = WN * NB * 32;
  const int tm = cdiv(p.M, BM), tn = cdiv(p.N, BN);
  const dim3 grid(tm * tn, batch);
  if (bkm) hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, MB, NB, BKT, true>), grid, dim3(256), 0, stream, p, tm, tn);
  else hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, MB, NB, BKT, false>), grid, dim3(256), 0, stream, p, tm, tn);
  return mdt_check_launch("gemm_f32");
}

// ------------------------------------------------------------------------------------------------------------------
// bf16x3: the Linear layers' C = A * B^T (+ bias) on fp32 operands at fp32-level accuracy on the bf16 matrix pipe (16x the
// fp32 one).  Every fp32 x splits EXACTLY into x = b0 + b1 + b2 (three bf16 terms of 8 significand bits each, fp32's
// exponent range: b0 = rne(x), b1 = rne(x - b0), b2 = x - b0 - b1), and of the nine products of two split operands the six
// with term indices summing to <= 2 are kept: a c = a0 c0 + (a0 c1 + a1 c0 + a0 c2 + a1 c1 + a2 c0) + O(2^-24 |a c|).  The
// main product a0 c0 has its own accumulator, so it rounds once per 16-k MFMA instead of once per k (mdt_gemm_f32's fma
// chain); the five corrections (~2^-8 of it) share a second one; the two are added once before the fp32 epilogue.
// Structure: 128 x 128 x 32 tile, 8 waves of 64 x 32 (two per SIMD), global loads staged in registers one K-tile ahead; a
// tile is split ONCE per element while it is written to LDS (three bf16 planes of [256 rows][32 k], 64-byte rows; 2 x 48 KiB
// double-buffered) and a fragment is one ds_read_b128 per plane.  v_mfma_f32_32x32x16_bf16 takes
// the B fragment first, as fmma does, so the accumulator layout is the one f32_epilogue consumes.  No atomics, no split-K:
// repeated runs give identical bits.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ unsigned x3_pk(float lo, float hi) {  // two RNE bf16 in one dword (v_cvt_pk_bf16_f32)
  const bf16x2 h = __builtin_convertvector((f32x2){lo, hi}, bf16x2);
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ f32x2 x3_unpk(unsigned w) {
  return (f32x2){__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}
#define X3_INLINE __attribute__((always_inline))  // (the K loop must not become calls)
__device__ __forceinline__ bool x3_finite(float v) { return fabsf(v) <= 3.4028235e38f; }  // false for inf and NaN

// eight consecutive k of one row -> the same 16 bytes of the three planes.  Not finite x: b1 = b2 = 0 (inf stays inf, NaN
// stays NaN); a finite x that RNE would round to inf: b0 rounds toward zero.  Both show as a non-finite x - b0.
__device__ __forceinline__ void x3_split8(const f32x4 v0, const f32x4 v1, u32x4& p0, u32x4& p1, u32x4& p2) {
  f32x2 x[4] = {(f32x2){v0[0], v0[1]}, (f32x2){v0[2], v0[3]}, (f32x2){v1[0], v1[1]}, (f32x2){v1[2], v1[3]}};
  unsigned w0[4];
  f32x2 r[4];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w0[j] = x3_pk(x[j][0], x[j][1]);
    r[j] = x[j] - x3_unpk(w0[j]);
    bad |= !x3_finite(r[j][0]) || !x3_finite(r[j][1]);
  }
  if (__any(bad)) {  // wave-uniform: a branch hipcc keeps, not selects on every element
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (x3_finite(r[j][e])) continue;
        const float xe = x[j][e];
        if (!x3_finite(xe)) {
          r[j][e] = 0.f;
        } else {
          const unsigned t = __float_as_uint(xe) >> 16;  // toward zero
          w0[j] = e ? (w0[j] & 0xffffu) | (t << 16) : (w0[j] & 0xffff0000u) | t;
          r[j][e] = xe - __uint_as_float(t << 16);
        }
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned w1 = x3_pk(r[j][0], r[j][1]);
    const f32x2 r2 = r[j] - x3_unpk(w1);
    p0[j] = w0[j];
    p1[j] = w1;
    p2[j] = x3_pk(r2[0], r2[1]);
  }
}

__global__ __launch_bounds__(512) void gemm_bf16x3_kernel(const Params p, const int tiles_m, const int tiles_n) {
  constexpr int NT = 512, WN = 4, MB = 2, NB = 1, BM = 128, BN = 128, BKT = 32;  // 8 waves (2 per SIMD) of 64 x 32
  constexpr int CPR = BKT / 8;                          // 16-byte chunks (8 k) per LDS row of a plane
  constexpr int CH = BM * CPR / NT;                     // chunks per thread and K-tile, of A and of B (BM == BN)
  constexpr int PLANE = (BM + BN) * CPR;                // 16-byte chunks of one plane of one buffer
  static_assert(CH >= 1 && BM == BN, "tile");
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][3][PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int nt = tiles_m * tiles_n;
  int t = blockIdx.x;
  {
    const int q = nt >> 3, r = nt & 7, x = t & 7, i = t >> 3;
    t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  constexpr int GM = 8;
  const int per_group = GM * tiles_n, grp = t / per_group, first_m = grp * GM;
  const int gm = min(tiles_m - first_m, GM), in_g = t - grp * per_group;
  const int tm = first_m + in_g % gm, tn = in_g / gm;
  const int m0 = tm * BM, n0 = tn * BN;

  f32x16 acc[MB][NB], cor[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = cor[i][j][e] = 0.f;

  // thread chunk q = tid + NT i: tile row q / CPR, k = 8 (q % CPR) .. + 7 as two 16-byte global loads; operand o = 0 (A)
  // / 1 (B).  Rows beyond M / N are clamped to the last row: they only feed output rows / columns that are never stored,
  // so the loads need no select (which would make the wave wait for them right away).
  f32x4 g[2][CH][2];
  const float* pg[2][CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int q = tid + NT * i, row = q / CPR, c = q % CPR;
    pg[0][i] = p.A + (long)min(m0 + row, p.M - 1) * p.lda + 8 * c;
    pg[1][i] = p.B + (long)min(n0 + row, p.N - 1) * p.ldb + 8 * c;
  }
  const bool k_ragged = (p.K % BKT) != 0;
  auto gload = [&](int k0) X3_INLINE {
    if (!k_ragged || k0 + BKT <= p.K) {
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) g[o][i][h] = *(const f32x4*)(pg[o][i] + k0 + 4 * h);
    } else {  // last, partial K-tile: the K tail reads as zeros (addresses clamped inside the operand rows)
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int c4 = 8 * ((tid + NT * i) % CPR) + 4 * h;
            const f32x4 v = *(const f32x4*)(pg[o][i] + 4 * h + min(k0, p.K - 4 - c4));
            g[o][i][h] = k0 + c4 < p.K ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
          }
    }
  };
  // chunk c of LDS row `row` (A rows 0 .. BM - 1, then B) sits at row * CPR + (c ^ ((row >> 2) & 3)): the 16 consecutive
  // rows of a fragment read's lane group land on 16 distinct 16-byte bank slots
  auto lstore = [&](int buf) X3_INLINE {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int q = tid + NT * i, row = q / CPR + o * BM, c = q % CPR;
        const int at = row * CPR + (c ^ ((row >> 2) & 3));
        u32x4 w0, w1, w2;
        x3_split8(g[o][i][0], g[o][i][1], w0, w1, w2);
        lds[buf][0][at] = w0;
        lds[buf][1][at] = w1;
        lds[buf][2][at] = w2;
      }
  };

  const int nk = (p.K + BKT - 1) / BKT;
  const int r = lane & 31, kh = lane >> 5;
  // fragments of k-step s (16 k) of the three planes: lane (r, kh) holds row r, k = 16 s + 8 kh .. + 7
  bf16x8 fa[3][MB], fb[3][NB];
  auto fload = [&](int buf, int s) X3_INLINE {
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const int row = (wm * MB + i) * 32 + r;
      const int at = row * CPR + ((2 * s + kh) ^ ((row >> 2) & 3));
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) fa[pl][i] = __builtin_bit_cast(bf16x8, lds[buf][pl][at]);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int row = BM + (wn * NB + i) * 32 + r;
      const int at = row * CPR + ((2 * s + kh) ^ ((row >> 2) & 3));
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) fb[pl][i] = __builtin_bit_cast(bf16x8, lds[buf][pl][at]);
    }
  };
  // six products per block and k-step; consecutive MFMAs go to different accumulators
  auto fmma = [&]() X3_INLINE {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int jj = 0; jj < NB; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[0][jj], fa[0][i], acc[i][jj], 0, 0, 0);
    constexpr int PB[5] = {0, 1, 0, 1, 2}, PA[5] = {1, 0, 2, 1, 0};  // (B plane, A plane) of the corrections
#pragma unroll
    for (int pr = 0; pr < 5; ++pr)
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int jj = 0; jj < NB; ++jj)
          cor[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[PB[pr]][jj], fa[PA[pr]][i], cor[i][jj], 0, 0, 0);
  };
  // K-tile kt (buffer kt & 1): the loads of tile kt + 1 are issued at the top and split into the other buffer after the
  // MFMAs -- that buffer held tile kt - 1, whose reads completed before the previous barrier (hipcc counts the waits).
  // Two waves per SIMD: one wave's split (VALU) and stores run under the other's MFMAs.
  auto step = [&](auto par_c, int kt) X3_INLINE {
    constexpr int par = decltype(par_c)::value;
    const bool more = kt + 1 < nk;
    if (more) gload((kt + 1) * BKT);
#pragma unroll
    for (int s = 0; s < BKT / 16; ++s) {
      fload(par, s);
      fmma();
    }
    if (more) lstore(par ^ 1);
    __syncthreads();
  };
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
  }
  // an inf operand makes the main sum inf; its corrections (inf times a small term of either sign, or 0) are dropped
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] += x3_finite(acc[i][j][e]) ? cor[i][j][e] : 0.f;
  f32_epilogue<MB, NB>(p, acc, m0, n0, wm, wn, r, kh, p.out);
}

// ------------------------------------------------------------------------------------------------------------------
// The autoencoder's 3x3 convolutions in the bf16x3 arithmetic, as an IMPLICIT GEMM: gemm_bf16x3_kernel (same tile, same
// split while staging, same six products on two accumulators, same epilogue -- its body restated, so that kernel's code does
// not change) whose A operand is gathered from the fp32 NHWC activation [B, Hi, Hi, C] instead of read from a matrix.  Row m
// of the product is output pixel (b, yo, xo); K runs over (ky, kx, c) and C % 32 == 0, so a 32-wide K-tile lies inside ONE
// tap.  A thread stages one 8-float chunk of ONE A row per K-tile: (b, yo, xo) are computed once, per K-tile only the tap
// changes, which gives a source pixel or -- for a padding tap -- the zero line of 32 floats in front of `act` (selected through
// the ADDRESS, so no load is followed by a select that would wait for it).  Row bases are 64-bit: no batch limit below
// M = B Ho Ho < 2^31.  Gather modes (geometry of mdt_conv3x3_nhwc / mdt_conv3x3_down_nhwc):
//   plain  mul 1, pad 1, sh 0: source (yo + ky - 1, xo + kx - 1), inside [0, Hi)
//   up     mul 1, pad 1, sh 1: the same in the nearest-2x image of side 2 Hi, source pixel = coordinate >> 1
//   down   mul 2, pad 0, sh 0: source (2 yo + ky, 2 xo + kx), row / column Hi reading zero (F.pad (0, 1, 0, 1), stride 2)
// B is the fp32 weight [Cout][9 C]; rows beyond M / N are clamped (never stored).  No atomics, no split-K.
struct ConvGeom {
  int Hi, C, Ho;        // input side, input channels, output side
  int mul, pad, sh;     // source coordinate = (out * mul + tap - pad), valid inside [0, lim), source pixel = coordinate >> sh
  int lim;
};

__global__ __launch_bounds__(512) void conv3x3_bf16x3_kernel(const Params p, const ConvGeom cg, const int tiles_m, const int tiles_n) {
  constexpr int NT = 512, WN = 4, MB = 2, NB = 1, BM = 128, BN = 128, BKT = 32;
  constexpr int CPR = BKT / 8;
  constexpr int PLANE = (BM + BN) * CPR;
  static_assert(BM * CPR == NT && BN * CPR == NT, "one A chunk and one B chunk per thread and K-tile");
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][3][PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int nt = tiles_m * tiles_n;
  int t = blockIdx.x;
  {
    const int q = nt >> 3, r = nt & 7, x = t & 7, i = t >> 3;
    t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  constexpr int GM = 8;
  const int per_group = GM * tiles_n, grp = t / per_group, first_m = grp * GM;
  const int gm = min(tiles_m - first_m, GM), in_g = t - grp * per_group;
  const int tm = first_m + in_g % gm, tn = in_g / gm;
  const int m0 = tm * BM, n0 = tn * BN;

  f32x16 acc[MB][NB], cor[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = cor[i][j][e] = 0.f;

  // this thread's chunk: tile row tid / CPR, floats 8 (tid % CPR) .. + 7 of the K-tile, of A (gathered) and of B
  const int srow = tid / CPR, sc = tid % CPR;
  const int m = min(m0 + srow, p.M - 1);
  const int hw = cg.Ho * cg.Ho;
  const int b = m / hw, pix = m - b * hw;
  const int yo = pix / cg.Ho, xo = pix - yo * cg.Ho;
  const int ybase = yo * cg.mul - cg.pad, xbase = xo * cg.mul - cg.pad;
  const float* const abase = p.A + (long)b * cg.Hi * cg.Hi * cg.C + 8 * sc;   // sample b, channel chunk of this thread
  const float* const azero = p.A - BKT + 8 * sc;                               // the zero line in front of the activation
  const float* const pb = p.B + (long)min(n0 + srow, p.N - 1) * p.ldb + 8 * sc;
  f32x4 g[2][2];
  int tap = 0, c0 = 0;  // (ky, kx) = (tap / 3, tap % 3) and first channel of the NEXT K-tile to load (wave-uniform)
  auto gload = [&](int k0) X3_INLINE {
    const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;  // tap / 3 for tap < 9
    const int yy = ybase + ky, xx = xbase + kx;
    const bool ok = (unsigned)yy < (unsigned)cg.lim && (unsigned)xx < (unsigned)cg.lim;
    const float* src = ok ? abase + ((long)((yy >> cg.sh) * cg.Hi + (xx >> cg.sh)) * cg.C + c0) : azero;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      g[0][h] = *(const f32x4*)(src + 4 * h);
      g[1][h] = *(const f32x4*)(pb + k0 + 4 * h);
    }
    c0 += BKT;
    if (c0 == cg.C) {
      c0 = 0;
      ++tap;
    }
  };
  auto lstore = [&](int buf) X3_INLINE {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int row = srow + o * BM;
      const int at = row * CPR + (sc ^ ((row >> 2) & 3));
      u32x4 w0, w1, w2;
      x3_split8(g[o][0], g[o][1], w0, w1, w2);
      lds[buf][0][at] = w0;
      lds[buf][1][at] = w1;
      lds[buf][2][at] = w2;
    }
  };

  const int nk = p.K / BKT;
  const int r = lane & 31, kh = lane >> 5;
  bf16x8 fa[3][MB], fb[3][NB];
  auto fload = [&](int buf, int s) X3_INLINE {
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const int row = (wm * MB + i) * 32 + r;
      const int at = row * CPR + ((2 * s + kh) ^ ((row >> 2) & 3));
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) fa[pl][i] = __builtin_bit_cast(bf16x8, lds[buf][pl][at]);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int row = BM + (wn * NB + i) * 32 + r;
      const int at = row * CPR + ((2 * s + kh) ^ ((row >> 2) & 3));
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) fb[pl][i] = __builtin_bit_cast(bf16x8, lds[buf][pl][at]);
    }
  };
  auto fmma = [&]() X3_INLINE {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int jj = 0; jj < NB; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[0][jj], fa[0][i], acc[i][jj], 0, 0, 0);
    constexpr int PB[5] = {0, 1, 0, 1, 2}, PA[5] = {1, 0, 2, 1, 0};
#pragma unroll
    for (int pr = 0; pr < 5; ++pr)
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int jj = 0; jj < NB; ++jj)
          cor[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[PB[pr]][jj], fa[PA[pr]][i], cor[i][jj], 0, 0, 0);
  };
  // the K loop of gemm_bf16x3_kernel (hipcc counts the waits)
  auto step = [&](auto par_c, int kt) X3_INLINE {
    constexpr int par = decltype(par_c)::value;
    const bool more = kt + 1 < nk;
    if (more) gload((kt + 1) * BKT);
#pragma unroll
    for (int s = 0; s < BKT / 16; ++s) {
      fload(par, s);
      fmma();
    }
    if (more) lstore(par ^ 1);
    __syncthreads();
  };
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
  }
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] += x3_finite(acc[i][j][e]) ? cor[i][j][e] : 0.f;
  f32_epilogue<MB, NB>(p, acc, m0, n0, wm, wn, r, kh, p.out);
}

// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_rows_f32_kernel(float* __restrict__ s, long R, int n, int n_valid, float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  float* r = s + row * n;
  // the row (1-4 KiB) stays in L1 / L2 over the three passes
  float mx = -3.0e38f;
  for (int i = lane; i < n_valid; i += 64) mx = fmaxf(mx, r[i] * scale);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int i = lane; i < n_valid; i += 64) sum += expf(r[i] * scale - mx);
  const float inv = 1.f / wave_sum(sum);
  for (int i = lane; i < n; i += 64) r[i] = i < n_valid ? expf(r[i] * scale - mx) * inv : 0.f;
}

// the same with the row in registers (n = 256 NV4 floats per row, one 16-byte access per lane and 256 columns): one read,
// one exp per element, one write -- the three-pass form above runs at 2.6 TB/s on 256-wide rows, this one at the
// streaming rate
template <int NV4>
__global__ __launch_bounds__(256) void softmax_rows_f32_reg_kernel(float* __restrict__ s, long R, float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  float* r = s + row * (256L * NV4);
  f32x4 v[NV4];
#pragma unroll
  for (int i = 0; i < NV4; ++i) v[i] = *(const f32x4*)(r + 4 * (lane + 64 * i));
  float mx = -3.0e38f;
#pragma unroll
  for (int i = 0; i < NV4; ++i) mx = fmaxf(fmaxf(mx, fmaxf(v[i][0], v[i][1])), fmaxf(v[i][2], v[i][3]));
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[i][e] = expf((v[i][e] - mx) * scale);
      sum += v[i][e];
    }
  const float inv = 1.f / wave_sum(sum);
#pragma unroll
  for (int i = 0; i < NV4; ++i) *(f32x4*)(r + 4 * (lane + 64 * i)) = (f32x4){v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv};
}

// ------------------------------------------------------------------------------------------------------------------
// Fused fp32 attention for L <= 256 tokens: one 8-wave workgroup per (sample, head), K and V of the item staged ONCE in
// LDS as fp32 rows (pitch HD + 4 floats: the 16 rows a ds_read_b128 lane group touches fall on 16 distinct 16-byte bank
// slots), a wave owns 32 queries.  Scores are computed TRANSPOSED -- S^T = K Q^T with v_mfma_f32_32x32x2_f32, K rows as the
// A operand from LDS, the wave's Q rows as the B operand from registers -- so a lane holds, for ITS query (column
// lane & 31), the scores of keys 32 kb + 8 (e / 4) + 4 (lane / 32) + e % 4: the softmax is a per-lane reduction plus one
// exchange with lane ^ 32, and the probabilities are ALREADY the B operand of O^T = V^T P^T (the two lane halves of
// accumulator register e are the two contraction slots of one MFMA; the matching V rows come from LDS as 4-byte reads,
// conflict-free).  Nothing but q, k, v is read and nothing but the output written: the three-launch form (q k^T -> HBM ->
// softmax -> HBM -> p v) moved 2.1 GB of scores per XL/2 layer at batch 128.
template <int HD, int L>
__global__ __launch_bounds__(512) void attn_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int H, float scale) {
  constexpr int HDP = HD + 4, KB = L / 32, NJ = HD / 8, NDB = (HD + 31) / 32, CPR = HD / 4;
  extern __shared__ __attribute__((aligned(16))) float attn_smem[];
  float* Ks = attn_smem;
  float* Vs = attn_smem + L * HDP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int W = H * HD;
  const long ld = 3L * W;
  const float* base = qkv + (long)b * L * ld + h * HD;
  constexpr int NCH = L * CPR, IT = (NCH + 511) / 512;
  {
    f32x4 kreg[IT], vreg[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = min(tid + 512 * i, NCH - 1), row = q / CPR, c = q - row * CPR;
      kreg[i] = *(const f32x4*)(base + row * ld + W + 4 * c);
      vreg[i] = *(const f32x4*)(base + row * ld + 2 * W + 4 * c);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = tid + 512 * i, row = q / CPR, c = q - row * CPR;
      if (q < NCH) {
        *(f32x4*)(Ks + row * HDP + 4 * c) = kreg[i];
        *(f32x4*)(Vs + row * HDP + 4 * c) = vreg[i];
      }
    }
  }
  const int r = lane & 31, kh = lane >> 5, q0 = wave * 32;
  f32x4 qf[NJ];
  {
    const float* qp = base + (long)min(q0 + r, L - 1) * ld + 4 * kh;
#pragma unroll
    for (int j = 0; j < NJ; ++j) qf[j] = *(const f32x4*)(qp + 8 * j);
  }
  __syncthreads();
  if (q0 >= L) return;
  f32x16 S[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
    for (int e = 0; e < 16; ++e) S[kb][e] = 0.f;
    const float* kp = Ks + (32 * kb + r) * HDP + 4 * kh;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x4 kf = *(const f32x4*)(kp + 8 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i) S[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qf[j][i], S[kb], 0, 0, 0);
    }
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, S[kb][e]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      S[kb][e] = expf((S[kb][e] - mx) * scale);
      sum += S[kb][e];
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.f / sum;
  f32x16 O[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[db][e] = 0.f;
  int dcol[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) dcol[db] = min(32 * db + r, HD - 1);  // (columns >= HD of the last block are never stored)
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float* vp = Vs + (32 * kb + 8 * (e >> 2) + 4 * kh + (e & 3)) * HDP;
#pragma unroll
      for (int db = 0; db < NDB; ++db) O[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[dcol[db]], S[kb][e], O[db], 0, 0, 0);
    }
  float* op = out + ((long)b * L + q0 + r) * W + h * HD;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int d0 = 32 * db + 8 * q4 + 4 * kh;
      if (d0 < HD)
        *(f32x4*)(op + d0) = (f32x4){O[db][4 * q4] * inv, O[db][4 * q4 + 1] * inv, O[db][4 * q4 + 2] * inv, O[db][4 * q4 + 3] * inv};
    }
}

template <int HD, int L>
int launch_attn(const float* qkv, float* out, int B, int H, hipStream_t stream) {
  constexpr int bytes = 2 * L * (HD + 4) * 4;
  static bool once = false;
  if (!once) {
    if (hipFuncSetAttribute((const void*)attn_f32_kernel<HD, L>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      mdt_set_error("attn_f32: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      return MDT_ERR_LAUNCH;
    }
    once = true;
  }
  const float scale = 1.f / sqrtf((float)HD);
  hipLaunchKernelGGL((attn_f32_kernel<HD, L>), dim3(B * H), dim3(512), bytes, stream, qkv, out, H, scale);
  return mdt_check_launch("attn_f32");
}

// one wave per row; NVT float4 per lane (branch-free, as norm.hip's bf16-output kernel)
template <int NVT>
__global__ __launch_bounds__(256) void ln_modulate_f32_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                              const float* __restrict__ scale, int mod_ld, int rows_per_sample,
                                                              float* __restrict__ xn, int M, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nv = D >> 2;
  const float* xr = x + (long)row * D;
  const long b = row / rows_per_sample;
  const float* sh = shift + b * mod_ld;
  const float* sc = scale + b * mod_ld;
  f32x4 v[NVT], a[NVT], m[NVT];
  int col[NVT];
  float own[NVT];
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    const int c = lane + 64 * i;
    own[i] = c < nv ? 1.f : 0.f;
    col[i] = 4 * min(c, nv - 1);
    v[i] = *(const f32x4*)(xr + col[i]);
    a[i] = *(const f32x4*)(sh + col[i]);
    m[i] = *(const f32x4*)(sc + col[i]);
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
  float* o = xn + (long)row * D;
#pragma unroll
  for (int i = 0; i < NVT; ++i) {
    f32x4 rr;
#pragma unroll
    for (int e = 0; e < 4; ++e) rr[e] = (v[i][e] - mean) * rstd * (1.f + m[i][e]) + a[i][e];
    *(f32x4*)(o + col[i]) = rr;
  }
}

__global__ void timestep_embed_f32_kernel(const float* __restrict__ t, float* __restrict__ out, int ld, int B, int dim) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (idx >= B * half) return;
  const int b = idx / half, i = idx - b * half;
  const float freq = expf(-logf(10000.f) * (float)i / (float)half);
  const float a = t[b] * freq;
  out[(long)b * ld + i] = cosf(a);
  out[(long)b * ld + half + i] = sinf(a);
}

__global__ void silu_f32_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = silu_f32(in[i]);
}

// out[(b, j), :] = in[(b, j), :] + rows[j, :]   (4 floats per thread)
__global__ void add_rows_f32_kernel(const float* __restrict__ in, const float* __restrict__ rows, float* __restrict__ out, long nq,
                                    int T, int Dq) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const long row = i / Dq;
  const int cq = (int)(i - row * Dq), j = (int)(row % T);
  const f32x4 a = *(const f32x4*)(in + 4 * i);
  const f32x4 b = *(const f32x4*)(rows + ((long)j * Dq + cq) * 4);
  *(f32x4*)(out + 4 * i) = (f32x4){a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]};
}

}  // namespace f32p

static f32p::Params f32_params(const mdt_gemm_f32_args* a, int heads) {
  f32p::Params p;
  p.A = a->A; p.lda = a->lda; p.B = a->B; p.ldb = a->ldb;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.bias = a->bias; p.epi = a->epi;
  p.out = a->out; p.ldo = a->ldo;
  p.res = a->res; p.ldres = a->ldres;
  p.gate = a->gate; p.gate_ld = a->gate_ld; p.rps = a->rows_per_sample > 0 ? a->rows_per_sample : 1;
  p.heads = heads;
  p.a_sb = a->a_stride_b; p.a_sh = a->a_stride_h; p.b_sb = a->b_stride_b; p.b_sh = a->b_stride_h;
  p.o_sb = a->o_stride_b; p.o_sh = a->o_stride_h;
  p.vec_ok = a->ldo % 4 == 0 && ((uintptr_t)a->out & 15) == 0 && (a->o_stride_b | a->o_stride_h) % 4 == 0 &&
             (!a->bias || ((uintptr_t)a->bias & 15) == 0) &&
             (!a->res || (a->ldres % 4 == 0 && ((uintptr_t)a->res & 15) == 0)) &&
             (!a->gate || (a->gate_ld % 4 == 0 && ((uintptr_t)a->gate & 15) == 0));
  p.dbg = 0;
  return p;
}

// The Linear layers of the bf16x3 plan (gemm_bf16x3_kernel): mdt_gemm_f32's contract without the batched / k-major forms
// -- attention stays exact fp32.
extern "C" int mdt_gemm_bf16x3(const mdt_gemm_f32_args* a, mdt_stream_t stream) {
  MDT_REQUIRE(a && a->A && a->B && a->out, "gemm_bf16x3: null pointer");
  MDT_REQUIRE(a->M > 0 && a->N > 0 && a->K >= 4 && a->K % 4 == 0, "gemm_bf16x3: M, N > 0 and K a positive multiple of 4");
  MDT_REQUIRE(a->batch <= 1 && a->heads <= 1 && !a->b_kmajor, "gemm_bf16x3: linear layers only (batched / k-major B: mdt_gemm_f32)");
  MDT_REQUIRE(a->lda % 4 == 0 && a->ldb % 4 == 0 && (((uintptr_t)a->A | (uintptr_t)a->B) & 15) == 0,
              "gemm_bf16x3: operand rows must be 16-byte aligned");
  MDT_REQUIRE(a->epi >= MDT_F32EPI_NONE && a->epi <= MDT_F32EPI_GATE_RES, "gemm_bf16x3: unknown epilogue");
  MDT_REQUIRE(a->epi != MDT_F32EPI_GATE_RES || (a->res && a->rows_per_sample > 0), "gemm_bf16x3: GATE_RES needs res and rows_per_sample");
  const long tm = cdiv(a->M, 128), tn = cdiv(a->N, 128);
  MDT_REQUIRE(tm * tn <= 2147483647L, "gemm_bf16x3: too many tiles");
  const f32p::Params p = f32_params(a, 1);
  hipLaunchKernelGGL(f32p::gemm_bf16x3_kernel, dim3((unsigned)(tm * tn)), dim3(512), 0, (hipStream_t)stream, p, (int)tm, (int)tn);
  return mdt_check_launch("gemm_bf16x3");
}

// The autoencoder's 3x3 convolutions of the 'bf16x3' arithmetic (conv3x3_bf16x3_kernel).
extern "C" int mdt_conv3x3_bf16x3_nhwc(const float* act, int B, int Hi, int C, int up, int down, const float* W, const float* bias,
                                       const float* res, float* out, long ldo, int Cout, mdt_stream_t stream) {
  MDT_REQUIRE(act && W && out, "conv3x3_bf16x3: null pointer");
  MDT_REQUIRE(B > 0 && Hi > 0 && Cout > 0 && C >= 32 && C % 32 == 0, "conv3x3_bf16x3: B, Hi, Cout > 0 and C a positive multiple of 32");
  MDT_REQUIRE((up == 0 || up == 1) && (down == 0 || down == 1) && !(up && down), "conv3x3_bf16x3: up and down are 0 or 1, not both");
  MDT_REQUIRE(!down || Hi % 2 == 0, "conv3x3_bf16x3: the stride-2 form needs an even input side");
  MDT_REQUIRE(Hi <= 16384 && 9L * C <= 2147483647L, "conv3x3_bf16x3: image side / channel count too large");
  MDT_REQUIRE(ldo >= Cout, "conv3x3_bf16x3: ldo < Cout");
  MDT_REQUIRE((((uintptr_t)act | (uintptr_t)W) & 15) == 0, "conv3x3_bf16x3: act and W must be 16-byte aligned");
  const int Ho = down ? Hi / 2 : Hi << up;
  const long M = (long)B * Ho * Ho;
  MDT_REQUIRE(M <= 2147483647L, "conv3x3_bf16x3: B * Ho * Ho must fit 31 bits");
  const long tm = cdiv(M, 128), tn = cdiv(Cout, 128);
  MDT_REQUIRE(tm * tn <= 2147483647L, "conv3x3_bf16x3: too many tiles");
  mdt_gemm_f32_args a = {};
  a.A = act; a.lda = C; a.B = W; a.ldb = 9L * C;
  a.M = (int)M; a.N = Cout; a.K = 9 * C;
  a.bias = bias; a.epi = res ? MDT_F32EPI_GATE_RES : MDT_F32EPI_NONE;  // gate NULL = 1: out = res + (acc + bias)
  a.out = out; a.ldo = ldo; a.res = res; a.ldres = ldo; a.rows_per_sample = 1;
  const f32p::Params p = f32_params(&a, 1);
  f32p::ConvGeom cg;
  cg.Hi = Hi; cg.C = C; cg.Ho = Ho;
  cg.mul = down ? 2 : 1; cg.pad = down ? 0 : 1; cg.sh = up; cg.lim = down ? Hi : Ho;
  hipLaunchKernelGGL(f32p::conv3x3_bf16x3_kernel, dim3((unsigned)(tm * tn)), dim3(512), 0, (hipStream_t)stream, p, cg, (int)tm, (int)tn);
  return mdt_check_launch("conv3x3_bf16x3");
}

extern "C" int mdt_gemm_f32(const mdt_gemm_f32_args* a, mdt_stream_t stream) {
  MDT_REQUIRE(a && a->A && a->B && a->out, "gemm_f32: null pointer");
  MDT_REQUIRE(a->M > 0 && a->N > 0 && a->K >= 4 && a->K % 4 == 0, "gemm_f32: M, N > 0 and K a positive multiple of 4");
  MDT_REQUIRE(a->lda % 4 == 0 && a->ldb % 4 == 0 && (((uintptr_t)a->A | (uintptr_t)a->B) & 15) == 0,
              "gemm_f32: operand rows must be 16-byte aligned");
  MDT_REQUIRE(a->epi >= MDT_F32EPI_NONE && a->epi <= MDT_F32EPI_GATE_RES, "gemm_f32: unknown epilogue");
  MDT_REQUIRE(a->epi != MDT_F32EPI_GATE_RES || (a->res && a->rows_per_sample > 0), "gemm_f32: GATE_RES needs res and rows_per_sample");
  const int batch = a->batch > 0 ? a->batch : 1;
  const int heads = a->heads > 0 ? a->heads : 1;
  MDT_REQUIRE(batch % heads == 0 && batch <= 65535, "gemm_f32: batch must be a multiple of heads and <= 65535");
  if (a->b_kmajor) MDT_REQUIRE(a->N % 4 == 0, "gemm_f32: k-major B needs N % 4 == 0");
  MDT_REQUIRE(((a->a_stride_b | a->a_stride_h | a->b_stride_b | a->b_stride_h) & 3) == 0, "gemm_f32: batch strides must be multiples of 4 elements");
  f32p::Params p = f32_params(a, heads);
#ifdef MDT_EXPERIMENTS
  {
    static int ablate = -1;
    if (ablate < 0) {
      const char* e = getenv("MDT_F32_ABLATE");
      ablate = e ? atoi(e) : 0;
    }
    p.dbg = ablate;
  }
#endif
  const hipStream_t st = (hipStream_t)stream;
  const bool bkm = a->b_kmajor != 0;
  // column tile: 128 unless the problem is narrower (attention's p v with N = head_dim).  (A 256 x 128 tile with 16-deep
  // K-tiles -- 23 instead of 31 operand bytes per kFLOP -- measured the same 0.65-0.71 of peak as this one,
  // profiles/r6_f32_bench_tiles.txt, and does not fit 256 registers with the two-ahead load staging: not instantiated.)
  // the LDS-DMA form for the Linear layers (MDT_F32_DMA=0: the register-staged form, A/B runs)
  static int dma_knob = -1;
  if (dma_knob < 0) {
    const char* e = getenv("MDT_F32_DMA");
    dma_knob = e ? atoi(e) : 1;
  }
  if (dma_knob && a->N > 64 && !bkm && batch == 1 && a->K % 32 == 0 && a->K >= 64 && a->M >= 128) {
    // (measured and not instantiated, profiles/r6_f32_dma_ab.txt: 256 x 128 x 16 tiles 4 % slower, 128 x 128 x 16 with up to
    // four workgroups per CU 11 % slower than this 128 x 128 x 32 form with two)
    const int tm = cdiv(p.M, 128), tn = cdiv(p.N, 128);
    hipLaunchKernelGGL((f32p::gemm_f32_dma_kernel<2, 2, 32, 2>), dim3(tm * tn), dim3(256), 0, st, p, tm, tn);
    return mdt_check_launch("gemm_f32 (LDS-DMA)");
  }
  if (a->N > 64) return f32p::launch<2, 2, 2, 2, 32>(p, bkm, batch, st);
  if (a->N > 32) return f32p::launch<4, 1, 1, 2, 32>(p, bkm, batch, st);
  return f32p::launch<4, 1, 1, 1, 32>(p, bkm, batch, st);
}

extern "C" int mdt_softmax_rows_f32(float* s, long R, int n, int n_valid, float scale, mdt_stream_t stream) {
  MDT_REQUIRE(s && R > 0 && n > 0 && n_valid > 0 && n_valid <= n, "softmax_rows_f32: bad arguments");
  MDT_REQUIRE(cdiv(R, 4) > 0 && R / 4 < 2147483647L, "softmax_rows_f32: too many rows");
  const dim3 grid(cdiv(R, 4)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (n_valid == n && n == 256) hipLaunchKernelGGL(f32p::softmax_rows_f32_reg_kernel<1>, grid, block, 0, st, s, R, scale);
  else if (n_valid == n && n == 512) hipLaunchKernelGGL(f32p::softmax_rows_f32_reg_kernel<2>, grid, block, 0, st, s, R, scale);
  else if (n_valid == n && n == 1024) hipLaunchKernelGGL(f32p::softmax_rows_f32_reg_kernel<4>, grid, block, 0, st, s, R, scale);
  else hipLaunchKernelGGL(f32p::softmax_rows_f32_kernel, grid, block, 0, st, s, R, n, n_valid, scale);
  return mdt_check_launch("softmax_rows_f32");
}

extern "C" int mdt_ln_modulate_f32(const float* x, const float* shift, const float* scale, int mod_ld, int rows_per_sample,
                                   float* xn, int M, int D, mdt_stream_t stream) {
  MDT_REQUIRE(x && shift && scale && xn, "ln_modulate_f32: null pointer");
  MDT_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1280 && M > 0 && rows_per_sample > 0 && mod_ld % 4 == 0, "ln_modulate_f32: bad shape");
  const dim3 grid(cdiv(M, 4)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (cdiv(D / 4, 64)) {
    case 1: hipLaunchKernelGGL(f32p::ln_modulate_f32_kernel<1>, grid, block, 0, st, x, shift, scale, mod_ld, rows_per_sample, xn, M, D); break;
    case 2: hipLaunchKernelGGL(f32p::ln_modulate_f32_kernel<2>, grid, block, 0, st, x, shift, scale, mod_ld, rows_per_sample, xn, M, D); break;
    case 3: hipLaunchKernelGGL(f32p::ln_modulate_f32_kernel<3>, grid, block, 0, st, x, shift, scale, mod_ld, rows_per_sample, xn, M, D); break;
    case 4: hipLaunchKernelGGL(f32p::ln_modulate_f32_kernel<4>, grid, block, 0, st, x, shift, scale, mod_ld, rows_per_sample, xn, M, D); break;
    default: hipLaunchKernelGGL(f32p::ln_modulate_f32_kernel<5>, grid, block, 0, st, x, shift, scale, mod_ld, rows_per_sample, xn, M, D); break;
  }
  return mdt_check_launch("ln_modulate_f32");
}

extern "C" int mdt_timestep_embed_f32(const float* t, float* out, int ld, int B, int dim, mdt_stream_t stream) {
  MDT_REQUIRE(t && out && dim % 2 == 0 && B > 0, "timestep_embed_f32: bad arguments");
  const int n = B * (dim / 2);
  hipLaunchKernelGGL(f32p::timestep_embed_f32_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, t, out, ld, B, dim);
  return mdt_check_launch("timestep_embed_f32");
}

extern "C" int mdt_silu_f32(const float* in, float* out, long n, mdt_stream_t stream) {
  MDT_REQUIRE(in && out && n > 0, "silu_f32: bad arguments");
  hipLaunchKernelGGL(f32p::silu_f32_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, in, out, n);
  return mdt_check_launch("silu_f32");
}

extern "C" int mdt_add_rows_f32(const float* in, const float* rows, float* out, long n_rows, int T, int D, mdt_stream_t stream) {
  MDT_REQUIRE(in && rows && out && n_rows > 0 && T > 0 && D > 0 && D % 4 == 0, "add_rows_f32: bad arguments");
  const long nq = n_rows * (D / 4);
  hipLaunchKernelGGL(f32p::add_rows_f32_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, in, rows, out, nq, T, D / 4);
  return mdt_check_launch("add_rows_f32");
}

// timm Attention (call site models/maskdit.py:178) in exact fp32 on the packed qkv buffer [B * L, 3 * H * hd]:
// out [B * L, H * hd] = softmax(q k^T hd^-0.5) v.  Fused single-launch kernel for L in {64, 256} and hd in {32, 64, 72}
// (every shipped 256^2-latent configuration); otherwise three launches through `scores_ws` (B * H * L * L floats):
// batched q k^T, in-place row softmax, batched p v.
static bool attn_f32_fused(int L, int hd) { return (L == 64 || L == 256) && (hd == 32 || hd == 64 || hd == 72); }

extern "C" long mdt_attn_f32_ws_floats(int B, int L, int H, int hd) {
  return attn_f32_fused(L, hd) ? 0L : (long)B * H * L * L;
}

extern "C" int mdt_attn_f32(const float* qkv, float* out, float* scores_ws, int B, int L, int H, int hd, mdt_stream_t stream) {
  MDT_REQUIRE(qkv && out && B > 0 && L > 0 && H > 0 && hd > 0 && hd % 4 == 0, "attn_f32: bad arguments");
  MDT_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0, "attn_f32: 16-byte aligned buffers");
  const hipStream_t st = (hipStream_t)stream;
  if (attn_f32_fused(L, hd) && (long)B * H < 2147483647L) {
#define ATTN_F32_GO(HDV, LV) return f32p::launch_attn<HDV, LV>(qkv, out, B, H, st);
    if (L == 256) { if (hd == 72) ATTN_F32_GO(72, 256) else if (hd == 64) ATTN_F32_GO(64, 256) else ATTN_F32_GO(32, 256) }
    else { if (hd == 72) ATTN_F32_GO(72, 64) else if (hd == 64) ATTN_F32_GO(64, 64) else ATTN_F32_GO(32, 64) }
#undef ATTN_F32_GO
  }
  MDT_REQUIRE(scores_ws, "attn_f32: this shape takes the three-launch form and needs scores_ws (mdt_attn_f32_ws_floats)");
  MDT_REQUIRE((long)B * H <= 65535, "attn_f32: batch * heads must not exceed 65535 in the three-launch form");
  const int W = H * hd;
  mdt_gemm_f32_args g = {};
  g.A = qkv; g.lda = 3L * W; g.B = qkv + W; g.ldb = 3L * W; g.b_kmajor = 0;
  g.M = L; g.N = L; g.K = hd; g.epi = MDT_F32EPI_NONE;
  g.out = scores_ws; g.ldo = L; g.batch = B * H; g.heads = H;
  g.a_stride_b = (long)L * 3 * W; g.a_stride_h = hd; g.b_stride_b = (long)L * 3 * W; g.b_stride_h = hd;
  g.o_stride_b = (long)H * L * L; g.o_stride_h = (long)L * L;
  int rc = mdt_gemm_f32(&g, stream);
  if (rc != MDT_OK) return rc;
  rc = mdt_softmax_rows_f32(scores_ws, (long)B * H * L, L, L, 1.f / sqrtf((float)hd), stream);
  if (rc != MDT_OK) return rc;
  mdt_gemm_f32_args v = {};
  v.A = scores_ws; v.lda = L; v.B = qkv + 2 * W; v.ldb = 3L * W; v.b_kmajor = 1;
  v.M = L; v.N = hd; v.K = L; v.epi = MDT_F32EPI_NONE;
  v.out = out; v.ldo = W; v.batch = B * H; v.heads = H;
  v.a_stride_b = (long)H * L * L; v.a_stride_h = (long)L * L; v.b_stride_b = (long)L * 3 * W; v.b_stride_h = hd;
  v.o_stride_b = (long)L * W; v.o_stride_h = hd;
  return mdt_gemm_f32(&v, stream);
}
