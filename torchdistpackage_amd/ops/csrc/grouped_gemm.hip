// Grouped expert GEMM over ragged token segments (gfx950) — the MoE expert
// FFN as ONE launch per GEMM for all local experts.
//
// Tokens are one row-major bf16 buffer whose rows are sorted by local
// expert; offs (E+1, int32|int64, DEVICE) holds the row offsets, expert e
// owns rows [offs[e], offs[e+1]).  Nothing here reads offs on the host: the
// grids come from T and E alone, so a captured launch stays valid while the
// routing (the contents of offs) changes.
//
//   fprop  y[seg_e]  = x[seg_e] @ w[e]^T + bias[e]   A k-inner, B k-inner
//   dgrad  dx[seg_e] = dy[seg_e] @ w[e]              A k-inner, B k-outer
//   wgrad  dw[e]     = dy[seg_e]^T @ x[seg_e]        A k-outer, B k-outer
//          db[e]     = sum_seg dy                    (plain two-stage column sum)
//
// The tile engine is gemm.hip's gemm256_kernel unchanged: 256x256 tile, 8
// waves (2Mx4N), 32-deep slots through a 4-slot LDS ring per operand, glds
// dwordx4 staging with the swizzle on the source address, tr16 gathers for
// the k-outer layouts, counted vmcnt waits (same number of glds per slot, so
// the wait arithmetic carries over), 16x16x32 bf16 MFMA, fp32 accumulate.
// What is new is everything ragged:
//
//  * fprop / dgrad: the grid has gg_row_tile_bound(T, E) * (N/256) blocks.
//    Each block finds its (expert, row tile) with gg_find_tile
//    (grouped_gemm_plan.h; a scan of offs from blockIdx, hence
//    wave-uniform); blocks beyond the last tile return as a whole before
//    any load or barrier.  A tile may own fewer than 256 rows: A-operand
//    source rows past the segment end are CLAMPED to the segment's last row
//    (in bounds, finite or not it only reaches accumulator rows that are
//    never stored) and stores are masked per row.
//  * wgrad: the reduction runs over the segment, any length.  The grid is
//    E * (Dout/256) * (Din/256).  Reduction rows past the segment end must
//    add exact zero (a clamped row would be added twice, the next segment's
//    row may hold anything), so their glds SOURCE points at a zeroed device
//    array instead — for both operands, 0 * NaN being NaN.  That also covers
//    the staging of slots beyond the last one, so no slot index is clamped
//    and a segment shorter than the ring depth is no special case.  An empty
//    segment skips the pipeline and stores the zero accumulators.
//
// Every offset is clamped to [0, T] before an address is formed.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "grouped_gemm_plan.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_v;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int SLOT_HW = 256 * 32;     // one staged slot: 8192 hw = 16 KiB
constexpr int BREG_HW = 4 * SLOT_HW;  // B operand region (halfwords)

#define GG_GLDS16(gp, lp)                                           \
  __builtin_amdgcn_global_load_lds(                                 \
      (const __attribute__((address_space(1))) unsigned int*)(gp),  \
      (__attribute__((address_space(3))) unsigned int*)(lp), 16, 0, 0)

// source of every wgrad reduction row past the segment end (512 B: one
// k-outer LDS row, so the redirected lanes stay coalesced)
__device__ __attribute__((aligned(16))) ushort gg_zero_row[256];

DEVINL unsigned gg_lds_addr_of(const ushort* p) {
  return (unsigned)(unsigned long long)(
      __attribute__((address_space(3))) const ushort*)p;
}

// bijective XCD-aware remap (gemm.hip T1)
DEVINL int gg_xcd_remap(int wg, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = wg & 7, idx = wg >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

DEVINL long gg_off(const void* offs, int offs64, int i, long T) {
  return offs64 ? gg_clamped((const long*)offs, i, T)
                : gg_clamped((const int*)offs, i, T);
}

template <int LAYA, int LAYB, bool WGRAD>
__launch_bounds__(512)
__global__ void ggemm256_kernel(const ushort* __restrict__ A,
                                const ushort* __restrict__ B,
                                const ushort* __restrict__ bias,
                                ushort* __restrict__ C,
                                const void* __restrict__ offs, int offs64,
                                int E, int T, int K,
                                long lda, long ldb, long ldc,
                                int tiles_m, int tiles_n, long wstride) {
  __shared__ __attribute__((aligned(16))) ushort lds[8 * SLOT_HW];  // 128 KiB

  const int wgid = gg_xcd_remap(blockIdx.x, gridDim.x);

  // ---- block -> tile (everything here derives from blockIdx and kernel
  // arguments: block-uniform)
  int expert, tn, row0 = 0, rows = 256, tm = 0;
  int k0 = 0, kend = 0, nslot;
  if (WGRAD) {
    // expert is the FASTEST index: an XCD's contiguous wgid chunk then
    // holds tiles of every expert, so one long segment (skewed routing)
    // spreads over all XCDs instead of serialising on one
    const int tile = wgid / E;
    expert = wgid - tile * E;
    tm = tile / tiles_n;
    tn = tile - tm * tiles_n;
    const long lo = gg_off(offs, offs64, expert, T);
    const long hi = gg_off(offs, offs64, expert + 1, T);
    k0 = (int)lo;
    kend = hi > lo ? (int)hi : k0;
    nslot = (kend - k0 + 31) / 32;
  } else {
    const long rt = wgid / tiles_n;
    tn = wgid - (int)rt * tiles_n;
    const GGTile t = offs64
        ? gg_find_tile((const long*)offs, E, (long)T, rt)
        : gg_find_tile((const int*)offs, E, (long)T, rt);
    if (t.expert < 0) return;   // surplus block: no load, no barrier yet
    expert = t.expert;
    row0 = t.row0;
    rows = t.rows;
    nslot = K / 32;
  }

  const int tid = threadIdx.x;
  const int w = tid >> 6;            // wave id (wave-uniform)
  const int lane = tid & 63;
  const int wm = w >> 2, wn = w & 3; // wave tile (wm*128, wn*64)
  const int l15 = lane & 15, lg = lane >> 4;

  const ushort* Abase;
  const ushort* Bbase;
  if (WGRAD) {
    Abase = A + tm * 256;                               // dy (T, Dout)
    Bbase = B + tn * 256;                               // x  (T, Din)
  } else {
    Abase = A + (long)row0 * lda;                       // segment rows
    const ushort* wexp = B + (long)expert * wstride;    // w[e] (Dout, Din)
    Bbase = (LAYB == 0) ? wexp + (long)(tn * 256) * ldb : wexp + tn * 256;
  }
  const int rmaxA = rows - 1;        // last A row this tile may read

  // ---- staging: 2 glds per thread per call (one 16 KiB slot).
  // ring = destination ring slot; ss = SOURCE slot.  fprop/dgrad clamp ss at
  // the tail (the target ring slot is no longer read); wgrad passes it
  // through, rows past the segment end read gg_zero_row.
  // guard = false (wgrad main loop only): the slot is known to lie wholly
  // inside the segment, no per-row select
  auto stage = [&](const ushort* gb, long ld, int ring, int ss, int region,
                   int lay, int rmax, bool guard) {
    const int kk = k0 + ss * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int dhw = region + ring * SLOT_HW + w * 512 + i * 4096;
      const ushort* g;
      if (lay == 0) {
        const int o = w * 1024 + i * 8192 + lane * 16;  // byte within slot
        const int row = o >> 6;                          // 64 B rows
        const int cs = (lane & 3) ^ (((row >> 2) & 1) << 1);
        const int srow = row < rmax ? row : rmax;
        g = gb + (long)srow * ld + kk + cs * 8;
      } else {
        const int o = w * 1024 + i * 8192 + lane * 16;
        const int krow = o >> 9;                         // 512 B rows
        const int c = lane & 31;
        const int cs = c ^ ((krow & 3) << 2);
        const bool live = !(WGRAD && guard) || kk + krow < kend;
        g = live ? gb + (long)(kk + krow) * ld + cs * 8
                 : gg_zero_row + c * 8;
      }
      GG_GLDS16(g, lds + dhw);
    }
  };
  auto src_slot = [&](int s) {
    return WGRAD ? s : (s < nslot ? s : nslot - 1);
  };
  auto stageA = [&](int s) {
    stage(Abase, lda, s & 3, src_slot(s), 0, LAYA, rmaxA, true);
  };
  auto stageB = [&](int s) {
    stage(Bbase, ldb, s & 3, src_slot(s), BREG_HW, LAYB, 255, true);
  };

  // ---- fragment reads (gemm.hip's maps)
  const int csr = lg ^ (((l15 >> 2) & 1) << 1);
  const int rdA = (wm * 128 + l15) * 32 + csr * 8;             // hw offset
  const int rdB = BREG_HW + (wn * 64 + l15) * 32 + csr * 8;
  const unsigned trlane = (unsigned)((8 * lg + ((lane >> 2) & 3)) * 512 +
                                     ((lane & 3) >> 1) * 16 + (lane & 1) * 8);
  const unsigned trJ = (unsigned)(((lane >> 2) & 3) << 6);
  const unsigned lds0 = gg_lds_addr_of(lds);

  // all of an operand's tr16 gathers in ONE asm block ending in the lgkm
  // wait (see gemm.hip: free-floating reads raced register moves)
  auto tr16x8 = [&](const unsigned* ad, bf16x8_v* fr, int n) {
    unsigned long long r[16];
    if (n == 8) {
      asm volatile(
          "ds_read_b64_tr_b16 %0, %16 offset:0\n\t"
          "ds_read_b64_tr_b16 %1, %16 offset:2048\n\t"
          "ds_read_b64_tr_b16 %2, %17 offset:0\n\t"
          "ds_read_b64_tr_b16 %3, %17 offset:2048\n\t"
          "ds_read_b64_tr_b16 %4, %18 offset:0\n\t"
          "ds_read_b64_tr_b16 %5, %18 offset:2048\n\t"
          "ds_read_b64_tr_b16 %6, %19 offset:0\n\t"
          "ds_read_b64_tr_b16 %7, %19 offset:2048\n\t"
          "ds_read_b64_tr_b16 %8, %20 offset:0\n\t"
          "ds_read_b64_tr_b16 %9, %20 offset:2048\n\t"
          "ds_read_b64_tr_b16 %10, %21 offset:0\n\t"
          "ds_read_b64_tr_b16 %11, %21 offset:2048\n\t"
          "ds_read_b64_tr_b16 %12, %22 offset:0\n\t"
          "ds_read_b64_tr_b16 %13, %22 offset:2048\n\t"
          "ds_read_b64_tr_b16 %14, %23 offset:0\n\t"
          "ds_read_b64_tr_b16 %15, %23 offset:2048\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]),
            "=&v"(r[4]), "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7]),
            "=&v"(r[8]), "=&v"(r[9]), "=&v"(r[10]), "=&v"(r[11]),
            "=&v"(r[12]), "=&v"(r[13]), "=&v"(r[14]), "=&v"(r[15])
          : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]),
            "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7]));
    } else {
      asm volatile(
          "ds_read_b64_tr_b16 %0, %8 offset:0\n\t"
          "ds_read_b64_tr_b16 %1, %8 offset:2048\n\t"
          "ds_read_b64_tr_b16 %2, %9 offset:0\n\t"
          "ds_read_b64_tr_b16 %3, %9 offset:2048\n\t"
          "ds_read_b64_tr_b16 %4, %10 offset:0\n\t"
          "ds_read_b64_tr_b16 %5, %10 offset:2048\n\t"
          "ds_read_b64_tr_b16 %6, %11 offset:0\n\t"
          "ds_read_b64_tr_b16 %7, %11 offset:2048\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]),
            "=&v"(r[4]), "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7])
          : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]));
    }
#pragma unroll
    for (int i = 0; i < n; ++i) {
      ((unsigned long long*)&fr[i])[0] = r[2 * i];
      ((unsigned long long*)&fr[i])[1] = r[2 * i + 1];
    }
  };
  auto trA_addr = [&](int ring, int mf) -> unsigned {
    const unsigned r16 = (unsigned)((wm * 128 + mf * 16) * 2);
    return lds0 + (unsigned)(ring * SLOT_HW * 2) + trlane + (r16 ^ trJ);
  };
  auto trB_addr = [&](int ring, int nf) -> unsigned {
    const unsigned r16 = (unsigned)((wn * 64 + nf * 16) * 2);
    return lds0 + (unsigned)(BREG_HW * 2) +
           (unsigned)(ring * SLOT_HW * 2) + trlane + (r16 ^ trJ);
  };
  auto readA0 = [&](int ring, int mf) -> bf16x8_v {
    return *(const bf16x8_v*)&lds[ring * SLOT_HW + rdA + mf * 512];
  };
  auto readB0 = [&](int ring, int nf) -> bf16x8_v {
    return *(const bf16x8_v*)&lds[ring * SLOT_HW + rdB + nf * 512];
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = (f32x4)(0.f);

  // one 32-deep slot (gemm.hip do_slot; wait_mode 0 / 1 = vmcnt(4) /
  // 2 = vmcnt(8))
  auto do_slot = [&](int s, int ring, bool stage_ok, int wait_mode,
                     bool guard) {
    const int nxt = WGRAD ? s + 3 : (stage_ok ? s + 3 : nslot - 1);
    stage(Abase, lda, (ring + 3) & 3, nxt, 0, LAYA, rmaxA, guard);
    bf16x8_v af[8], bfr[4];
    if (LAYA == 0) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) af[mf] = readA0(ring, mf);
    } else {
      unsigned ad[8];
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) ad[mf] = trA_addr(ring, mf);
      tr16x8(ad, af, 8);
    }
    if (LAYB == 0) {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) bfr[nf] = readB0(ring, nf);
    } else {
      unsigned ad[4];
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) ad[nf] = trB_addr(ring, nf);
      tr16x8(ad, bfr, 4);
    }
    stage(Bbase, ldb, (ring + 3) & 3, nxt, BREG_HW, LAYB, 255, guard);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      acc[mf][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af[mf], bfr[0], acc[mf][0], 0, 0, 0);
      acc[mf][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af[mf], bfr[1], acc[mf][1], 0, 0, 0);
    }
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      acc[mf][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af[mf], bfr[2], acc[mf][2], 0, 0, 0);
      acc[mf][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af[mf], bfr[3], acc[mf][3], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    if (wait_mode == 1)
      asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else if (wait_mode == 2)
      asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    else
      asm volatile("s_barrier" ::: "memory");
  };

  // nslot == 0 only for an empty wgrad segment (block-uniform): no staging,
  // the zero accumulators are the result
  if (nslot > 0) {
    // ---- prologue: slots 0..2 staged; wait until slot 0 landed
    stageA(0); stageB(0);
    stageA(1); stageB(1);
    stageA(2); stageB(2);
    asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");

    // ---- main loop: 4-slot groups (compile-time ring ids).  It stages
    // slots up to ns_main + 2; wgrad keeps that below the last slot, the
    // only one a segment can fill partly, so the loop stages unguarded
    const int ns_main = WGRAD ? (nslot > 4 ? (nslot - 4) & ~3 : 0)
                              : (nslot > 3 ? (nslot - 3) & ~3 : 0);
    int s = 0;
    for (; s < ns_main; s += 4) {
      do_slot(s, 0, true, 1, false);
      do_slot(s + 1, 1, true, 0, false);
      do_slot(s + 2, 2, true, 1, false);
      do_slot(s + 3, 3, true, 1, false);
    }
    for (; s < nslot; ++s)
      do_slot(s, s & 3, s + 3 < nslot, 2, true);
    // the tail's surplus glds target this block's LDS: drain them before
    // the block may end
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

  // ---- epilogue
  if (WGRAD) {
    ushort* Ce = C + (long)expert * wstride;            // dw[e] (Dout, Din)
    const int crow0 = tm * 256 + wm * 128;
    const int ccol0 = tn * 256 + wn * 64;
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      const int col = ccol0 + nf * 16 + l15;
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
        const long row = crow0 + mf * 16 + lg * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Ce[(row + r) * ldc + col] = f2bf(acc[mf][nf][r]);
      }
    }
  } else {
    const int ccol0 = tn * 256 + wn * 64;
    const ushort* be = bias ? bias + (long)expert * (tiles_n * 256) : nullptr;
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      const int col = ccol0 + nf * 16 + l15;
      const float bv = be ? bf2f(be[col]) : 0.f;
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
        const int lrow = wm * 128 + mf * 16 + lg * 4;   // row within tile
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (lrow + r < rows)                          // per-row mask
            C[((long)row0 + lrow + r) * ldc + col] =
                f2bf(acc[mf][nf][r] + bv);
      }
    }
  }
}

// db[e] = column sums of dy over segment e, fp32 accumulate, in two fixed-
// order stages (no atomics, so the result does not depend on timing):
// stage 1 cuts every segment into GG_DB_SPLIT row chunks — sized on the
// device from offs — and writes one fp32 partial row per chunk; block = 64
// column pairs x 8 row lanes, grid (N/128, E, GG_DB_SPLIT).  Stage 2 adds
// the partials in chunk order and rounds once.
constexpr int GG_DB_SPLIT = 16;

__global__ void gg_bias_grad_partial_kernel(const ushort* __restrict__ dy,
                                            const void* __restrict__ offs,
                                            int offs64, int T, int N,
                                            float* __restrict__ part) {
  __shared__ float red[8][128];
  const int e = blockIdx.y, z = blockIdx.z;
  const long lo = gg_off(offs, offs64, e, T);
  const long hi = gg_off(offs, offs64, e + 1, T);
  const long c = hi > lo ? hi - lo : 0;
  const long chunk = (c + GG_DB_SPLIT - 1) / GG_DB_SPLIT;
  const long r0 = lo + z * chunk;
  const long r1 = r0 + chunk < lo + c ? r0 + chunk : lo + c;
  const int cp = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 128 + cp * 2;      // N % 128 == 0
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
  for (long r = r0 + rl; r < r1; r += 8) {
    const unsigned v = *(const unsigned*)(dy + r * N + col);
    s0 += bf2f((unsigned short)(v & 0xffffu));
    s1 += bf2f((unsigned short)(v >> 16));
  }
  red[rl][cp * 2] = s0;
  red[rl][cp * 2 + 1] = s1;
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int i = 1; i < 8; ++i) {
      s0 += red[i][cp * 2];
      s1 += red[i][cp * 2 + 1];
    }
    float* p = part + ((long)e * GG_DB_SPLIT + z) * N + col;
    p[0] = s0;
    p[1] = s1;
  }
}

__global__ void gg_bias_grad_reduce_kernel(const float* __restrict__ part,
                                           ushort* __restrict__ db, int E,
                                           int N) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)E * N) return;
  const long e = i / N, col = i - e * N;
  float s = 0.f;
#pragma unroll
  for (int z = 0; z < GG_DB_SPLIT; ++z)
    s += part[(e * GG_DB_SPLIT + z) * N + col];
  db[i] = f2bf(s);
}

struct GGArgs { int E, T, Dout, Din, offs64; };

GGArgs gg_check(const torch::Tensor& tok, const char* tok_name, long tok_cols,
                const torch::Tensor& offs, long E, long Dout, long Din) {
  TORCH_CHECK(tok.is_cuda() && tok.scalar_type() == torch::kBFloat16 &&
              tok.dim() == 2 && tok.is_contiguous(), tok_name,
              " must be contiguous 2-D bf16 CUDA");
  TORCH_CHECK(tok.size(1) == tok_cols, tok_name, ": ", tok.size(1),
              " columns, expected ", tok_cols);
  TORCH_CHECK(offs.is_cuda() && offs.dim() == 1 && offs.is_contiguous() &&
              (offs.scalar_type() == torch::kInt ||
               offs.scalar_type() == torch::kLong),
              "offs must be a contiguous 1-D int32/int64 CUDA tensor");
  TORCH_CHECK(E >= 1 && offs.numel() == E + 1, "offs must have E+1 = ",
              E + 1, " entries, got ", offs.numel());
  TORCH_CHECK(Dout > 0 && Din > 0 && Dout % 256 == 0 && Din % 256 == 0,
              "grouped_gemm: Dout and Din must be multiples of 256 (got ",
              Dout, ", ", Din, ") — the dispatch layer should fall back");
  TORCH_CHECK(tok.size(0) < (1L << 31) - 512, "grouped_gemm: too many rows");
  return GGArgs{(int)E, (int)tok.size(0), (int)Dout, (int)Din,
                offs.scalar_type() == torch::kLong ? 1 : 0};
}

void check_w(const torch::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
              w.dim() == 3 && w.is_contiguous(),
              "w must be contiguous (E, Dout, Din) bf16 CUDA");
}

}  // namespace

// y (T,Dout): y[seg_e] = x[seg_e] @ w[e]^T + bias[e]; bias added in fp32
// before the single rounding.
torch::Tensor grouped_gemm_fprop(torch::Tensor x, torch::Tensor w,
                                 torch::Tensor offs,
                                 c10::optional<torch::Tensor> bias) {
  check_w(w);
  const GGArgs a = gg_check(x, "x", w.size(2), offs, w.size(0), w.size(1),
                            w.size(2));
  const ushort* bptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kBFloat16 &&
                bias->is_contiguous() && bias->dim() == 2 &&
                bias->size(0) == a.E && bias->size(1) == a.Dout,
                "bias must be contiguous (E, Dout) bf16 CUDA");
    bptr = (const ushort*)bias->data_ptr();
  }
  auto y = torch::empty({a.T, a.Dout}, x.options());
  if (a.T == 0) return y;
  const int tiles_n = a.Dout / 256;
  const long nwg = gg_row_tile_bound(a.T, a.E) * tiles_n;
  TORCH_CHECK(nwg < (1L << 31), "grouped_gemm: grid too large");
  hipLaunchKernelGGL((ggemm256_kernel<0, 0, false>), dim3((unsigned)nwg),
                     dim3(512), 0, at::cuda::getCurrentHIPStream(),
                     (const ushort*)x.data_ptr(), (const ushort*)w.data_ptr(),
                     bptr, (ushort*)y.data_ptr(), offs.data_ptr(), a.offs64,
                     a.E, a.T, a.Din, (long)a.Din, (long)a.Din, (long)a.Dout,
                     0, tiles_n, (long)a.Dout * a.Din);
  HIP_CHECK_LAST();
  return y;
}

// dx (T,Din): dx[seg_e] = dy[seg_e] @ w[e].
torch::Tensor grouped_gemm_dgrad(torch::Tensor dy, torch::Tensor w,
                                 torch::Tensor offs) {
  check_w(w);
  const GGArgs a = gg_check(dy, "dy", w.size(1), offs, w.size(0), w.size(1),
                            w.size(2));
  auto dx = torch::empty({a.T, a.Din}, dy.options());
  if (a.T == 0) return dx;
  const int tiles_n = a.Din / 256;
  const long nwg = gg_row_tile_bound(a.T, a.E) * tiles_n;
  TORCH_CHECK(nwg < (1L << 31), "grouped_gemm: grid too large");
  hipLaunchKernelGGL((ggemm256_kernel<0, 1, false>), dim3((unsigned)nwg),
                     dim3(512), 0, at::cuda::getCurrentHIPStream(),
                     (const ushort*)dy.data_ptr(),
                     (const ushort*)w.data_ptr(), nullptr,
                     (ushort*)dx.data_ptr(), offs.data_ptr(), a.offs64,
                     a.E, a.T, a.Dout, (long)a.Dout, (long)a.Din,
                     (long)a.Din, 0, tiles_n, (long)a.Dout * a.Din);
  HIP_CHECK_LAST();
  return dx;
}

// dw (E,Dout,Din): dw[e] = dy[seg_e]^T @ x[seg_e]; db (E,Dout) = column sums
// of dy per segment (fp32 accumulate), or None.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> grouped_gemm_wgrad(
    torch::Tensor dy, torch::Tensor x, torch::Tensor offs,
    bool want_bias_grad) {
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && dy.size(0) == x.size(0),
              "dy (T,Dout) and x (T,Din) must share T");
  const long E = offs.numel() - 1;
  const GGArgs a = gg_check(dy, "dy", dy.size(1), offs, E, dy.size(1),
                            x.size(1));
  gg_check(x, "x", x.size(1), offs, E, dy.size(1), x.size(1));
  c10::optional<torch::Tensor> db;
  if (a.T == 0) {
    if (want_bias_grad) db = torch::zeros({a.E, a.Dout}, dy.options());
    return {torch::zeros({a.E, a.Dout, a.Din}, dy.options()), db};
  }
  auto dw = torch::empty({a.E, a.Dout, a.Din}, dy.options());
  const int tiles_m = a.Dout / 256, tiles_n = a.Din / 256;
  const long nwg = (long)a.E * tiles_m * tiles_n;
  TORCH_CHECK(nwg < (1L << 31), "grouped_gemm: grid too large");
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((ggemm256_kernel<1, 1, true>), dim3((unsigned)nwg),
                     dim3(512), 0, stream,
                     (const ushort*)dy.data_ptr(),
                     (const ushort*)x.data_ptr(), nullptr,
                     (ushort*)dw.data_ptr(), offs.data_ptr(), a.offs64,
                     a.E, a.T, 0, (long)a.Dout, (long)a.Din, (long)a.Din,
                     tiles_m, tiles_n, (long)a.Dout * a.Din);
  HIP_CHECK_LAST();
  if (want_bias_grad) {
    db = torch::empty({a.E, a.Dout}, dy.options());
    auto part = torch::empty({a.E, GG_DB_SPLIT, a.Dout},
                             dy.options().dtype(torch::kFloat));
    hipLaunchKernelGGL(gg_bias_grad_partial_kernel,
                       dim3(a.Dout / 128, a.E, GG_DB_SPLIT), dim3(512), 0,
                       stream, (const ushort*)dy.data_ptr(), offs.data_ptr(),
                       a.offs64, a.T, a.Dout, part.data_ptr<float>());
    const long n = (long)a.E * a.Dout;
    hipLaunchKernelGGL(gg_bias_grad_reduce_kernel, dim3((n + 255) / 256),
                       dim3(256), 0, stream, part.data_ptr<float>(),
                       (ushort*)db->data_ptr(), a.E, a.Dout);
    HIP_CHECK_LAST();
  }
  return {dw, db};
}

// Host run of the kernels' block -> tile mapping: one row per row-tile index
// below the launch bound, (expert, first row, row count), expert -1 = idle.
torch::Tensor grouped_gemm_plan(torch::Tensor offs_cpu, int64_t T) {
  TORCH_CHECK(!offs_cpu.is_cuda() && offs_cpu.dim() == 1 &&
              offs_cpu.numel() >= 2 &&
              (offs_cpu.scalar_type() == torch::kInt ||
               offs_cpu.scalar_type() == torch::kLong),
              "offs_cpu must be a 1-D int32/int64 CPU tensor of E+1 entries");
  TORCH_CHECK(T >= 0 && T < (1L << 31) - 512, "T out of range");
  auto o = offs_cpu.contiguous();
  const int E = (int)o.numel() - 1;
  const long R = gg_row_tile_bound(T, E);
  auto plan = torch::empty({R, 3}, torch::dtype(torch::kLong));
  auto* p = plan.data_ptr<int64_t>();
  for (long rt = 0; rt < R; ++rt) {
    const GGTile t = o.scalar_type() == torch::kLong
        ? gg_find_tile((const long*)o.data_ptr<int64_t>(), E, (long)T, rt)
        : gg_find_tile(o.data_ptr<int>(), E, (long)T, rt);
    p[3 * rt] = t.expert;
    p[3 * rt + 1] = t.row0;
    p[3 * rt + 2] = t.rows;
  }
  return plan;
}
