// Weight-only int4 small-M linear for decode ("W4A16"), group-wise scales:
//   y[m,n] = bf16( sum_g scale[n,g] * sum_{k in g} q[n,k] * x[m,k] + bias[n] )
// q int4 in [-8,7], two per byte in a uint8 (N, K/2) tensor: byte b of a row
// holds k = 2b in its low nibble and k = 2b+1 in its high nibble, two's
// complement.  scale fp32 (N, K/128), x / bias / y bf16, 1 <= M <= 32.
//
// Two arms: a dot2 arm for M <= 2 (further down) and, for every other M, an
// arm on v_mfma_f32_16x16x32_bf16:
//  - x is the A operand (16 rows of m x 32 k), W^T the B operand (32 k x 16
//    n).  Lane l holds B for column n = l & 15 and its four C values are rows
//    m = (l >> 4) * 4 + r of the same column, so a group's scale multiplies
//    the lane's own accumulators: no shuffle, no reduction inside the wave.
//  - a lane's 16-byte load is 32 consecutive k of its row n, the k-group
//    kg = l >> 4 of a 128-wide scale group.  Dword i of the load is the B
//    fragment of MFMA i (k = 32 kg + 8 i + j), so four MFMAs into a zeroed
//    temporary cover exactly one scale group: acc += scale * tmp.
//  - int4 -> bf16 once per weight in registers, shared by all M rows:
//    sign-extending bit-field extract, int -> fp32, one packed fp32 -> bf16
//    convert per pair.  |q| <= 8 has 4 significant bits: exact.
//  - a workgroup is W = 4 or 8 waves over the SAME 16 output rows; wave w
//    takes the scale groups g = w (mod W) of every x tile, and the W partial
//    sums meet in LDS at the end.  N / 16 workgroups of W waves keep the grid
//    of a rows-per-wave kernel while a wave's B fragment serves 16 rows.  W =
//    8 where N / 16 workgroups alone would leave the chip short of waves.
//  - x is staged once per workgroup and tile in LDS as 16-byte units ordered
//    [k / 8][m], M rows only (dynamic LDS): the 16 lanes of a k-group read 16
//    consecutive units, conflict-free without padding.  Rows m >= M of the A
//    operand are zeros made in registers and are never read from anywhere.
//  - a tile's weight and scale loads are issued before the tile's x is staged,
//    so the stream overlaps the staging; at W = 4, 64 B (M <= 16) or 32 B
//    (M > 16) of weights per lane in flight, the int8 kernel's figures; at
//    W = 8 half of that in twice the waves.
//  - rows past N re-read row N - 1 and are never stored; every address is
//    formed from clamped indices.  No atomics, no scratch, no workspace:
//    pointers and sizes only, capturable into the decode hipGraph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

// no packed-fp32 VALU forms in this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

// a grid below this many workgroups runs 8 waves per workgroup instead of 4
// (two workgroups per CU of the 256).  The constant rests on one A/B run that
// was not recorded (w2 at M = 1: 29.8 us at 4 waves, 22.2 us at 8).
#define GEMV4_WIDE_BELOW 512
#define GEMV4_ROWS 16    // output rows per workgroup (one MFMA n tile)
#define GEMV4_GROUP 128  // k per scale group = k per wave step

typedef __attribute__((ext_vector_type(8))) __bf16 g4_bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 g4_bf16x2;
typedef __attribute__((ext_vector_type(2))) float g4_f32x2;
typedef __attribute__((ext_vector_type(4))) float g4_f32x4;

// eight int4 (one dword, k ascending from the low nibble) -> one B fragment
DEVINL g4_bf16x8 cvt8_i4_bf16(unsigned int w) {
  union { g4_bf16x2 v[4]; g4_bf16x8 f; } u;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // shift-left / arithmetic-shift-right pairs fold into one v_bfe_i32
    const float lo = (float)((int)(w << (28 - 8 * p)) >> 28);
    const float hi = (float)((int)(w << (24 - 8 * p)) >> 28);
    u.v[p] = __builtin_convertvector(g4_f32x2{lo, hi}, g4_bf16x2);
  }
  return u.f;
}

// all waves of a workgroup are on rows 16 * blockIdx.x + {0..15}
template <int MTILES, int WAVES>
__global__ __launch_bounds__(WAVES * WAVE) void gemv_w4a16_kernel(
    const ushort* __restrict__ x, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, const ushort* __restrict__ bias,
    ushort* __restrict__ y, int M, long N, long K, int has_bias) {
  // x tile: 64 KB of LDS at the largest M of either instantiation
  constexpr int KT = (MTILES == 1) ? 2048 : 1024;
  constexpr int G = KT / GEMV4_GROUP / WAVES;        // groups per wave, tile
  extern __shared__ uint4 xs[];                      // [KT / 8][M] units
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15;
  const int kg = lane >> 4;
  const long n0 = (long)blockIdx.x * GEMV4_ROWS;
  const long nc = min(n0 + l15, N - 1);   // a row past N re-reads row N - 1
  const long ngroups = K / GEMV4_GROUP;
  const unsigned char* qrow = q + nc * (K / 2) + kg * 16;
  const float* srow = scale + nc * ngroups;

  g4_f32x4 acc[MTILES];
#pragma unroll
  for (int t = 0; t < MTILES; ++t) acc[t] = (g4_f32x4)(0.f);

  for (long k0 = 0; k0 < K; k0 += KT) {
    const int kt = (int)min((long)KT, K - k0);
    const int tg = kt / GEMV4_GROUP;      // scale groups in this tile
    const long g0 = k0 / GEMV4_GROUP;
    // the tile's weights and scales first: in flight while x is staged
    uint4 w[G];
    float s[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int gi = wave + WAVES * j;          // wave-uniform
      if (gi < tg) {
        w[j] = *(const uint4*)&qrow[(g0 + gi) * (GEMV4_GROUP / 2)];
        s[j] = srow[g0 + gi];
      }
    }
    // cooperative x stage, 16-byte units: 8 consecutive threads take 8
    // consecutive units of one row (a full 128-byte line), then the next row
    const int units = kt / 8;             // a multiple of 16
    for (int i = threadIdx.x; i < M * units; i += WAVES * WAVE) {
      const int clo = i & 7, rest = i >> 3;
      const int chi = rest / M, m = rest - chi * M;
      const int c = chi * 8 + clo;
      xs[c * M + m] = *(const uint4*)&x[(long)m * K + k0 + c * 8];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int gi = wave + WAVES * j;
      if (gi < tg) {
        const unsigned int wd[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
        g4_f32x4 tmp[MTILES];
#pragma unroll
        for (int t = 0; t < MTILES; ++t) tmp[t] = (g4_f32x4)(0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const g4_bf16x8 b = cvt8_i4_bf16(wd[i]);
          const int c = gi * 16 + kg * 4 + i;         // unit of k = 8 c
#pragma unroll
          for (int t = 0; t < MTILES; ++t) {
            const int m = t * 16 + l15;
            union { uint4 u; g4_bf16x8 f; } a;
            a.u = xs[c * M + min(m, M - 1)];
            if (m >= M) a.u = make_uint4(0u, 0u, 0u, 0u);
            tmp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.f, b, tmp[t],
                                                             0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < MTILES; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(s[j], tmp[t][r],
                                                       acc[t][r]);
      }
    }
    __syncthreads();
  }
  // the waves' partial sums meet in LDS, over the x tile (free after the
  // loop's last barrier; the launcher sizes it for this too); thread
  // (r, lane) of the first four waves owns C register r of every M tile
  float (*red)[MTILES * 4][WAVE] = (float (*)[MTILES * 4][WAVE])xs;
#pragma unroll
  for (int t = 0; t < MTILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t * 4 + r][lane] = acc[t][r];
  __syncthreads();
  const int r = wave;
  const long n = n0 + l15;
  if (n >= N || r >= 4) return;
  const float b = has_bias ? bf2f(bias[n]) : 0.f;
#pragma unroll
  for (int t = 0; t < MTILES; ++t) {
    const int m = t * 16 + kg * 4 + r;
    if (m < M) {
      float v = red[0][t * 4 + r][lane];
#pragma unroll
      for (int w2 = 1; w2 < WAVES; ++w2) v += red[w2][t * 4 + r][lane];
      y[(long)m * N + n] = f2bf(v + b);
    }
  }
}

// ---- dot2 arm for tiny M, built the way gemv_int8.hip is: a wave owns 2
// output rows, a lane's 16-byte load is 32 consecutive k of a row (inside one
// scale group, so the group's scale folds into the lane's own partial sum:
// acc += scale * tmp), the x rows are staged in LDS row-major, products go
// through v_dot2_f32_bf16 and the wave reduces at the end.  A wave covers
// 2048 k per load; the x tile is 4096 k, two loads per row in flight (64 B
// per lane, the int8 kernel's figure).
#define GEMV4D_BLOCK 256
#define GEMV4D_WSTEP (WAVE * 32)
typedef short g4_s16x2 __attribute__((ext_vector_type(2)));

template <int MT>
__global__ __launch_bounds__(GEMV4D_BLOCK) void gemv_w4a16_dot2_kernel(
    const ushort* __restrict__ x, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, const ushort* __restrict__ bias,
    ushort* __restrict__ y, int M, long N, long K, int has_bias) {
  constexpr int R = 2, KT = 4096, NCH = KT / GEMV4D_WSTEP;
  __shared__ ushort xs[MT * KT];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long n0 = ((long)blockIdx.x * 4 + wave) * R;
  const bool live = n0 < N;
  const long ngroups = K / GEMV4_GROUP;
  float acc[R][MT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  for (long k0 = 0; k0 < K; k0 += KT) {
    const int kt = (int)min((long)KT, K - k0);   // a multiple of 128
    uint4 w[R][NCH];
    float s[R][NCH];
    if (live) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        // a row past N re-reads row n0; its sums are never stored
        const long nr = (n0 + r < N) ? n0 + r : n0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int kk = c * GEMV4D_WSTEP + lane * 32;
          if (kk < kt) {
            w[r][c] = *(const uint4*)&q[nr * (K / 2) + (k0 + kk) / 2];
            s[r][c] = scale[nr * ngroups + (k0 + kk) / GEMV4_GROUP];
          }
        }
      }
    }
    for (int i = threadIdx.x * 8; i < M * kt; i += GEMV4D_BLOCK * 8) {
      const int m = i / kt, c = i % kt;
      *(uint4*)&xs[m * KT + c] = *(const uint4*)&x[(long)m * K + k0 + c];
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int kk = c * GEMV4D_WSTEP + lane * 32;
        if (kk < kt) {
          union { g4_bf16x8 f; g4_s16x2 p[4]; } b[R][4];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            b[r][0].f = cvt8_i4_bf16(w[r][c].x);
            b[r][1].f = cvt8_i4_bf16(w[r][c].y);
            b[r][2].f = cvt8_i4_bf16(w[r][c].z);
            b[r][3].f = cvt8_i4_bf16(w[r][c].w);
          }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            if (m < M) {
              float tmp[R];
#pragma unroll
              for (int r = 0; r < R; ++r) tmp[r] = 0.f;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                union { uint4 u; g4_s16x2 p[4]; } a;
                a.u = *(const uint4*)&xs[m * KT + kk + 8 * i];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                  for (int r = 0; r < R; ++r)
                    tmp[r] = __builtin_amdgcn_fdot2_f32_bf16(
                        b[r][i].p[j], a.p[j], tmp[r], false);
              }
#pragma unroll
              for (int r = 0; r < R; ++r)
                acc[r][m] = fmaf(s[r][c], tmp[r], acc[r][m]);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = wave_sum(acc[r][m]);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (n0 + r < N) {
        const float b = has_bias ? bf2f(bias[n0 + r]) : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < M) y[(long)m * N + n0 + r] = f2bf(acc[r][m] + b);
      }
    }
  }
}

#pragma clang attribute pop

// The crossover: the dot2 arm serves M <= GEMV4_DOT2_MAX_M.  Forced through
// the binding (profiles/int4_gemv_kbench_arms.log, columns mfma / dot2) it is
// faster at M = 1 at all eight shapes (w2 14.2 against 20.0 us), faster or
// level at M = 2, slower at M = 4 at six of eight.
// arm: 0 = as dispatched, 1 = the MFMA arm, 2 = the dot2 arm (M <= 4 only);
// 1 and 2 are for the kbench columns and the tests
#define GEMV4_DOT2_MAX_M 2

torch::Tensor gemv_w4a16(torch::Tensor x, torch::Tensor q,
                         torch::Tensor scale,
                         c10::optional<torch::Tensor> bias, int64_t arm) {
  TORCH_CHECK(x.is_cuda() && q.is_cuda() && scale.is_cuda(),
              "gemv_w4a16: device tensors only");
  TORCH_CHECK(x.is_contiguous() && q.is_contiguous() &&
              scale.is_contiguous(), "gemv_w4a16: contiguous operands only");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "gemv_w4a16: x is bf16");
  TORCH_CHECK(q.scalar_type() == torch::kByte,
              "gemv_w4a16: q is uint8 (two int4 per byte)");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat,
              "gemv_w4a16: scale is fp32");
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && scale.dim() == 2 &&
              x.size(1) == 2 * q.size(1),
              "gemv_w4a16: x (M,K), q (N,K/2), scale (N,K/128)");
  const int M = (int)x.size(0);
  const long N = q.size(0), K = x.size(1);
  TORCH_CHECK(N >= 1 && K >= GEMV4_GROUP && K % GEMV4_GROUP == 0,
              "gemv_w4a16: K must be a multiple of 128");
  TORCH_CHECK(scale.size(0) == N && scale.size(1) == K / GEMV4_GROUP,
              "gemv_w4a16: one scale per output row and group of 128");
  TORCH_CHECK(M >= 1 && M <= 32, "gemv_w4a16 is the M<=32 decode path");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
              (uintptr_t)q.data_ptr() % 16 == 0,
              "gemv_w4a16: x and q must be 16-byte aligned");
  const ushort* bptr = nullptr;
  int has_bias = 0;
  if (bias.has_value() && bias->numel() > 0) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                bias->scalar_type() == torch::kBFloat16 &&
                bias->numel() == N,
                "gemv_w4a16: bias is contiguous bf16 with N elements");
    bptr = (const ushort*)bias->data_ptr();
    has_bias = 1;
  }
  auto y = torch::empty({M, N}, x.options());
  const dim3 grid((unsigned)((N + GEMV4_ROWS - 1) / GEMV4_ROWS));
  auto stream = at::cuda::getCurrentHIPStream();
  const ushort* xp = (const ushort*)x.data_ptr();
  const unsigned char* qp = (const unsigned char*)q.data_ptr();
  const float* sp = (const float*)scale.data_ptr();
  ushort* yp = (ushort*)y.data_ptr();
  TORCH_CHECK(arm >= 0 && arm <= 2 && (arm != 2 || M <= 4),
              "gemv_w4a16: arm is 0, 1 or 2 (2: M <= 4)");
  if (arm == 2 || (arm == 0 && M <= GEMV4_DOT2_MAX_M)) {
    const dim3 dgrid((unsigned)((N + 7) / 8));
#define LAUNCH_D(MT_)                                                        \
  hipLaunchKernelGGL((gemv_w4a16_dot2_kernel<MT_>), dgrid,                   \
                     dim3(GEMV4D_BLOCK), 0, stream, xp, qp, sp, bptr, yp, M, \
                     N, K, has_bias)
    if (M == 1) LAUNCH_D(1);
    else if (M == 2) LAUNCH_D(2);
    else LAUNCH_D(4);
#undef LAUNCH_D
    TORCH_CHECK(hipGetLastError() == hipSuccess);
    return y;
  }
  // LDS: the x tile holds M rows only, M * KT bf16 (at most 64 KB), and is
  // reused for the waves' partial sums, WAVES * MTILES * 4 * 64 floats
#define LAUNCH(MT_, W_, KT_)                                                 \
  hipLaunchKernelGGL((gemv_w4a16_kernel<MT_, W_>), grid, dim3(W_ * WAVE),    \
                     std::max((size_t)M * KT_ * 2, (size_t)W_ * MT_ * 1024), \
                     stream, xp, qp, sp, bptr, yp, M, N, K, has_bias)
  const bool wide = grid.x < GEMV4_WIDE_BELOW;
  if (M <= 16) {
    if (wide) LAUNCH(1, 8, 2048); else LAUNCH(1, 4, 2048);
  } else {
    if (wide) LAUNCH(2, 8, 1024); else LAUNCH(2, 4, 1024);
  }
#undef LAUNCH
  TORCH_CHECK(hipGetLastError() == hipSuccess);
  return y;
}
