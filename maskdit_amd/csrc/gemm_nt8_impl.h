// gemm_nt8: the large-problem bf16 NT GEMM (C[M,N] = A[M,K] * B[N,K]^T + fused epilogue).
//
// 256 x (64*NF) output tile per 512-thread workgroup (8 waves as 2(M) x 4(N); each wave owns
// 128 x 16*NF = 8 x NF MFMA 16x16x32 fragments), K-step 64, ONE workgroup per CU.
// Pipeline (per K-tile 4 phases, one raw s_barrier each, no vmcnt(0) in steady state):
//
//   * operands go HBM -> LDS by 16-byte LDS-DMA (global_load_lds) into a 2-stage ring; the ring
//     is managed at SLOT granularity: A slot p = the 2 x 32 tile rows the two wave-rows consume
//     in phase p (exactly one LDS-DMA instruction per wave), B = NF instructions per wave.
//     A slot is refilled with K-tile t+2 in the phase right after its last ds_read retired, so
//     every load has ~6 phases (1.5 K-tiles of MFMA work) to land;
//   * phase g: the 4*NF MFMAs of phase g with ONE memory instruction pinned behind each of the first ones
//              (sched_barrier): the ds_reads of phase g+1's fragments into the alternate register set, then the
//              LDS-DMA refill of the slot read during phase g-1 (round 3; round 2 clustered reads / DMA / MFMAs: both
//              waves of a SIMD then queue memory instructions in front of an idle matrix pipe, -13 % on the K loop);
//              s_waitcnt vmcnt(W_p) lgkmcnt(0) ; s_barrier
//     W_p = number of loads issued after the one that the NEXT phase's reads depend on (loads
//     retire in order), computed at compile time -- never 0 until the last two K-tiles;
//   * XOR-swizzled LDS image through the *source* address (LDS-DMA destinations are lane-linear),
//     conflict-free ds_read_b128 fragment reads; XCD-aware tile order;
//   * PERSISTENT: one workgroup per CU walks the tile list; when a tile's K loop ends, the first
//     two K-tiles of the workgroup's NEXT output tile are put in flight before the epilogue runs;
//   * EPILOGUE (round 2): the MFMAs are issued with the operands SWAPPED (D^T = B A^T), so a lane's four
//     accumulator registers of a fragment are four CONSECUTIVE COLUMNS of one output row (row = lane & 15,
//     columns 4*(lane>>4)..+3): the fused epilogue works straight out of the accumulators with 16-byte fp32 /
//     8-byte bf16 global accesses (bf16 pairs of fragments are widened to 16 bytes with v_permlane16_swap) --
//     no LDS restaging, no barrier, no LDS region.  The epilogue class is a TEMPLATE parameter and every
//     global load of the tile (residual / saved pre-activation, gates, bias) is issued up front (a
//     DEPTH-band look-ahead bounded by the register file), so the tile pays ONE memory round trip and its
//     stores stream out back to back instead of one load->store round trip per 16-row band.
//
// Requirements (checked by the dispatcher in gemm.hip): M % (128*WR) == 0, N % (64*NF) == 0,
// K % 128 == 0, 16-byte aligned rows of every output.  Everything else runs the 128x128 kernel in gemm.hip.
#pragma once
#ifndef NT8_DEFAULT_SCHED
#define NT8_DEFAULT_SCHED 5  // one memory instruction behind each MFMA: +8..11 % on the K loop over the clustered form (round 3)
#endif
#include "common.h"
#include "../../include/maskdit_hip.h"
#include "gemm_common.h"
#include <type_traits>

// an all-zero row standing in for a NULL bias (the epilogue's loads are unconditional)
#define NT8_ZERO_ROW 1024
static __device__ float nt8_zero_row[NT8_ZERO_ROW + 64];  // zero-initialised; one copy per translation unit

// timing stamps of the experiment kernels (SCHED bit 9; tools/nt8_stamps.py): [tile][event] shader-clock values of wave 0
// of workgroup 0 -- 0 tile start (after the tile-top wait + barrier), 1 K loop done, 2 next tile's LDS-DMA issued,
// 3 epilogue's last store issued
static __device__ unsigned long long nt8_stamps[2 * 64 * 4];  // [wave 0 | last wave]

namespace nt8 {

enum { E_PLAIN = 0, E_F32 = 1, E_ACT = 2, E_GATE = 3, E_DACT = 4,
       E_TRK = 5 };  // E_TRK: overlap EXPERIMENT (tools/nt8_bench.py): GATE-sized epilogue traffic issued one 16-byte op per
                     // phase inside the K loop instead of after it (results are garbage; timing only)

// loads issued per wave in phase p: one A slot + RPP B rounds while p < NF (RPP = 1 with 8 waves,
// 2 with 4 waves: half as many waves share the same B tile)
constexpr int c_issue(int p, int NF, int RPP) { return 1 + (p < NF ? RPP : 0); }

// steady-state vmcnt operand at the end of phase p (see header)
constexpr int wait_count(int p, int NF, int RPP, int trk = 0) {
  // next phase (g+1) prefetches A slot (p+2)&3 [of the current or the next K-tile], issued at
  // phase g-6 whose phase index is (p+2)&3; the B instruction of that phase was issued after it.
  int w = (((p + 2) & 3) < NF) ? RPP : 0;
  for (int d = 5; d >= 0; --d) w += c_issue(((p - d) % 4 + 4) % 4, NF, RPP) + trk;  // trk extra ops per phase (E_TRK)
  if (p == 2) {
    // phase 3 also reads the whole next-tile B: its last instruction was issued at phase NF-1 of
    // the previous K-tile; after it: one A load per phase NF..3, then phases 0..2 of this tile
    int wb = (4 - NF) + c_issue(0, NF, RPP) + c_issue(1, NF, RPP) + c_issue(2, NF, RPP) + trk * ((4 - NF) + 3);
    if (wb < w) w = wb;
  }
  return w;
}

// vmcnt operand at the end of phase d (0..7) of the LAST pair of K-tiles, where nothing is issued any
// more: the steady-state count minus the loads those phases would have issued
constexpr int drain_count(int d, int NF, int RPP) {
  if (d >= 6) return 0;  // nothing left to fetch: only LDS reads remain
  int w = (((d + 2) & 3) < NF) ? RPP : 0;                        // B issued right after the awaited A load (phase -6+d)
  for (int e = d - 5; e < 0; ++e) w += c_issue(((e % 4) + 4) % 4, NF, RPP);  // steady phases after it
  if (d == 2) {
    int wb = 4 - NF;  // A loads issued after the last B instruction of the final K-tile
    if (wb < w) w = wb;
  }
  return w;
}

// s_waitcnt vmcnt(N) lgkmcnt(0) as the BUILTIN (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8]
// | vmcnt_hi[15:14]) so that hipcc's own waitcnt bookkeeping sees the LDS reads as retired and
// does not re-wait (lgkmcnt(0)) in front of the next phase's MFMAs; the empty asm statements pin
// the memory-operation order around it.
template <int N> __device__ __forceinline__ void wait_vm_lgkm() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("; MDT_CHK hand_wait" ::: "memory");  // (a comment in the ISA: tools/check_waits.py audits the immediate that follows)
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (0 << 8) | ((N >> 4) << 14));
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  bf16x2 t;
  t[0] = f2bf(lo);
  t[1] = f2bf(hi);
  return __builtin_bit_cast(unsigned, t);
}
__device__ __forceinline__ f32x4 round_bf16(f32x4 v) {
  return (f32x4){bf2f(f2bf(v[0])), bf2f(f2bf(v[1])), bf2f(f2bf(v[2])), bf2f(f2bf(v[3]))};
}
__device__ __forceinline__ f32x4 unpack_bf16x4(uint2 u) {
  bf16x2 a = __builtin_bit_cast(bf16x2, u.x), b = __builtin_bit_cast(bf16x2, u.y);
  return (f32x4){bf2f(a[0]), bf2f(a[1]), bf2f(b[0]), bf2f(b[1])};
}

// Store one 16-row band of a wave's tile as bf16.  y[j] = this lane's 4 consecutive columns of fragment j
// (columns 16j + 4g .. +3 of row `fr`, g = lane >> 4).  `ub` = wave-uniform address of the band's first row at
// the wave tile's column 0; `lo_pair` / `lo_tail` = this lane's byte offsets (bf16_lane_offsets).  Fragment pairs
// (j, j+1) are exchanged between the odd and even 16-lane rows with v_permlane16_swap so that every lane stores
// 8 consecutive columns (16 bytes): even g -> fragment j columns 4g..4g+7, odd g -> fragment j+1 columns
// 4(g-1)..4(g-1)+7.
// For an ODD fragment count the last fragment of band i (8 bytes per lane) is not stored on its own: it is carried to
// band i + 1 and exchanged with that band's last fragment the same way, so that ONE 16-byte store per lane writes both
// (even 16-lane rows: 8 columns of band i's row, odd rows: 8 columns of band i + 1's row; `lo_tail2` = bf16_tail2_offset
// relative to the EVEN band).  8-byte accesses run at 0.54-0.70 of the 16-byte rate: 12 instead of 16 store instructions
// per wave and 256 x 192 tile.
struct TailCarry { unsigned lo, hi; };
template <int NF, bool ODD_BAND>
__device__ __forceinline__ void store_band_bf16(char* ub, char* ub_even, unsigned lo_pair, unsigned lo_tail2, const f32x4* y, TailCarry& tc) {
  unsigned lo[NF], hi[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    lo[j] = pack_bf16x2(y[j][0], y[j][1]);
    hi[j] = pack_bf16x2(y[j][2], y[j][3]);
  }
#pragma unroll
  for (int j = 0; j + 1 < NF; j += 2) {
    auto a = __builtin_amdgcn_permlane16_swap(lo[j], lo[j + 1], false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi[j], hi[j + 1], false, false);
    *(uint4*)(ub + opaque(lo_pair) + 32 * j) = make_uint4(a[0], b[0], a[1], b[1]);
  }
  if (NF & 1) {
    if (!ODD_BAND) {
      tc.lo = lo[NF - 1];
      tc.hi = hi[NF - 1];
    } else {
      auto a = __builtin_amdgcn_permlane16_swap(tc.lo, lo[NF - 1], false, false);
      auto b = __builtin_amdgcn_permlane16_swap(tc.hi, hi[NF - 1], false, false);
      *(uint4*)(ub_even + opaque(lo_tail2) + 32 * (NF - 1)) = make_uint4(a[0], b[0], a[1], b[1]);
    }
  }
}
// band i of a [rows, ld] bf16 array at wave-uniform base `base0` (band 0): the constant-index wrapper the epilogues use
#define NT8_STORE_BAND(NFV, base0, ld, i, lp, lt2, y, tc)                                                     \
  do {                                                                                                       \
    if ((i) & 1) store_band_bf16<NFV, true>(band(base0, (i), (ld), 2), band(base0, (i) - 1, (ld), 2), lp, lt2, y, tc); \
    else store_band_bf16<NFV, false>(band(base0, (i), (ld), 2), band(base0, (i), (ld), 2), lp, lt2, y, tc);   \
  } while (0)
// (measured and dropped, round 3: whole-128-byte-line stores for NF = 4 -- the second 64-byte piece of a row rotated by 8
// lanes with DPP row_ror:8 so that one instruction writes 8 rows x 128 B.  tools/micro/store_bench.hip: a lone CU writes
// 64-byte segments at <= 24 GB/s and whole lines at >= 51 GB/s, but inside this epilogue nothing moved (1156 vs 1164 us at
// 256 CUs, 4.5 vs 4.75 us per tile at 128 CUs, with or without a half-period workgroup stagger: gpurun_out/r3/nt8_lines2.log)
// -- with every CU in its epilogue at once the stores run at the chip's HBM write rate, 5-6 TB/s.)
// The inverse of store_band_bf16: load one 16-row band of a bf16 array as 16 bytes per lane (8 consecutive columns of a
// fragment pair; 8 bytes for an odd last fragment) and hand every lane the 4 columns per fragment the accumulators use
// (v_permlane16_swap is its own inverse on a pair).  Half as many load instructions as one 8-byte load per fragment --
// 8-byte accesses run at 0.54-0.70 of the 16-byte rate (MI355X_MICROARCH.md).  raw[] is kept in the packed form so that
// the look-ahead costs the same registers as before.
template <int NF> struct BandRaw {
  uint4 pr[NF / 2 > 0 ? NF / 2 : 1];
  uint2 tail;
};
template <int NF> __device__ __forceinline__ void load_band_bf16(BandRaw<NF>& r, const char* ub, unsigned lo_pair, unsigned lo_tail) {
#pragma unroll
  for (int j = 0; j + 1 < NF; j += 2) r.pr[j / 2] = *(const uint4*)(ub + opaque(lo_pair) + 32 * j);
  if (NF & 1) r.tail = *(const uint2*)(ub + opaque(lo_tail) + 32 * (NF - 1));
}
template <int NF> __device__ __forceinline__ void unpack_band_bf16(const BandRaw<NF>& r, f32x4* h) {
#pragma unroll
  for (int j = 0; j + 1 < NF; j += 2) {
    const uint4 x = r.pr[j / 2];  // (a0, b0, a1, b1) of store_band_bf16
    auto l = __builtin_amdgcn_permlane16_swap(x.x, x.z, false, false);
    auto hh = __builtin_amdgcn_permlane16_swap(x.y, x.w, false, false);
    h[j] = unpack_bf16x4(make_uint2(l[0], hh[0]));
    h[j + 1] = unpack_bf16x4(make_uint2(l[1], hh[1]));
  }
  if (NF & 1) h[NF - 1] = unpack_bf16x4(r.tail);
}

// lane byte offsets into a bf16 [rows, ld] array for store_band_bf16 (fr = lane & 15, fg = lane >> 4)
__device__ __forceinline__ unsigned bf16_pair_offset(int fr, int fg, int ld) {
  return (unsigned)(fr * ld + ((fg & 1) ? 16 + 4 * (fg - 1) : 4 * fg)) * 2u;
}
__device__ __forceinline__ unsigned bf16_tail_offset(int fr, int fg, int ld) { return (unsigned)(fr * ld + 4 * fg) * 2u; }
// paired tail store (store_band_bf16): even 16-lane rows write band i's row fr, odd rows band i + 1's row fr (+ 16 rows)
__device__ __forceinline__ unsigned bf16_tail2_offset(int fr, int fg, int ld) {
  return (unsigned)((fr + ((fg & 1) ? 16 : 0)) * ld + ((fg & 1) ? 4 * (fg - 1) : 4 * fg)) * 2u;
}

// look-ahead (in 16-row bands) of the epilogue's row-dependent loads: as deep as the register file allows
constexpr int epi_depth(int E, int NF) {
  return E == E_DACT ? (NF >= 4 ? 4 : 8) : 0;
}

}  // namespace nt8

// WR = wave rows: 2 -> 256-row tile, 8 waves, one workgroup per CU (next-tile prefetch under the
// epilogue); 1 -> 128-row tile, 4 waves, TWO independent workgroups per CU, so one workgroup's
// epilogue (an HBM-write burst with idle matrix cores) runs under the other's K loop.
// SCHED = placement of the LDS-DMA refills (and fragment reads) inside a phase -- see PAIR_BODY; bit 4 = the
// round-2 addressing (per-lane 64-bit address arithmetic in the K loop) for A/B runs.
template <int NF, int WR, int E, int SCHED = NT8_DEFAULT_SCHED>
__global__ __launch_bounds__(256 * WR, 2) void gemm_nt8_kernel(NTParams p) {
#include "gemm_nt8_kbody.h"
}

// implicit-GEMM convolution with stride 2 (the encoder's Downsample, mdt_conv3x3_down_nhwc): the same body under a kernel
// name of its own -- 256-row tiles, fp32 class, SCHED = the conv bits (4096, + 8192 for the fused epilogue) + bit 14.  The
// body is shared TEXTUALLY so that gemm_nt8_kernel's code is untouched (tools/isa_diff.py: a shared device function
// changed the ISA of every instantiation) and the product library's gemm_nt8_kernel set stays the one
// tests/test_capi_cpu.py pins.
template <int NF, int SCHED_CONV>
__global__ __launch_bounds__(512, 2) void gemm_nt8_conv_down_kernel(NTParams p) {
  constexpr int WR = 2, E = 1, SCHED = SCHED_CONV | 16384;
#include "gemm_nt8_kbody.h"
}

int nt8_num_cus();

// one translation unit per epilogue class (gemm_nt8_c<class>.hip: #define NT8_CLASS <0..4>, then include this
// header and expand NT8_INSTANTIATE_CLASS) -- the five classes compile in parallel
#define NT8_CAT_(a, b) a##b
#define NT8_CAT(a, b) NT8_CAT_(a, b)
#define NT8_INST(NF, WR) template __global__ void gemm_nt8_kernel<NF, WR, NT8_CLASS>(NTParams);
#define NT8_LAUNCH(NF, WR) hipLaunchKernelGGL((gemm_nt8_kernel<NF, WR, NT8_CLASS>), dim3(grid), blk, 0, stream, p)
// NT8_WIDE = 1: the class has a 256 x 256 (NF = 4) instantiation (E_GATE keeps a 5-band residual look-ahead in
// registers next to the accumulators and stops at NF = 3)
#define NT8_INSTANTIATE_CLASS(NT8_WIDE, NT8_WIDE_INST)                                                            \
  NT8_INST(2, 2) NT8_INST(3, 2) NT8_INST(2, 1) NT8_INST(3, 1)                                       \
  NT8_WIDE_INST                                                                                     \
  int NT8_CAT(launch_gemm_nt8_class, NT8_CLASS)(const NTParams& p, int nf, int wr, hipStream_t stream) { \
    const int bm = 128 * wr;                                                                        \
    const int ntiles = (p.M / bm) * (p.N / (64 * nf));                                              \
    const int slots = nt8_num_cus() * (wr == 1 ? 2 : 1);                                            \
    const int grid = ntiles < slots ? ntiles : slots;                                               \
    const dim3 blk(256 * wr);                                                                       \
    if (nf == 4 && !(NT8_WIDE && wr == 2)) {                                                        \
      mdt_set_error("gemm_nt8: no 256-column instantiation for this epilogue class");               \
      return MDT_ERR_ARG;                                                                           \
    }                                                                                               \
    if (wr == 2) {                                                                                  \
      switch (nf) {                                                                                 \
        case 2: NT8_LAUNCH(2, 2); break;                                                            \
        case 3: NT8_LAUNCH(3, 2); break;                                                            \
        default: NT8_LAUNCH((NT8_WIDE ? 4 : 2), 2); break;                                          \
      }                                                                                             \
    } else {                                                                                        \
      if (nf == 3) NT8_LAUNCH(3, 1);                                                                \
      else NT8_LAUNCH(2, 1);                                                                        \
    }                                                                                               \
    return mdt_check_launch("gemm_nt8");                                                            \
  }
