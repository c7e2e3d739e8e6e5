// Weight-only int8 GEMV for decode ("W8A16"):
//   y[m,n] = bf16( scale[n] * sum_k q[n,k] * x[m,k] + bias[n] )
// q int8 (N,K) in [-127,127], scale fp32 (N,), x / bias / y bf16.
//
// Same streaming design as gemv.hip: a wave owns R output rows, the x rows
// are staged once per workgroup through LDS as bf16, products accumulate in
// fp32 via v_dot2_f32_bf16.  What changes:
//  - a 16-byte load carries 16 weights, so a lane's K step is 16 and the
//    wave's is 1024.  To keep the bytes in flight per lane of the bf16 kernel
//    (2 rows x 2 loads) every lane loads ALL its chunks of the x tile,
//    KT / 1024 per row, before the tile's x is staged and the barrier is
//    passed: the weight stream overlaps the staging instead of following it.
//  - int8 -> bf16 happens in registers, once per weight, and is reused by
//    all M rows.  |q| <= 127 has 7 significant bits, bf16 keeps 8, so the
//    upper half of the converted fp32 IS the bf16 value: no rounding.
//  - scale[n] multiplies the wave-reduced fp32 sum once; bias is added in
//    fp32 and the result rounds to bf16 once.
//
// M <= 32, K % 16 == 0, row-major contiguous operands, x and q 16-byte
// aligned.  Pointers and sizes only: capturable into the decode hipGraph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

#define GEMV8_BLOCK 256  // 4 waves; wave w owns rows R*(blockIdx.x*4+w)+{0..R-1}
#define GEMV8_WSTEP (WAVE * 16)  // K covered by one 16-byte load per lane

typedef short sv2_i8 __attribute__((ext_vector_type(2)));
typedef float f2_i8 __attribute__((ext_vector_type(2)));
typedef __bf16 bf2_i8 __attribute__((ext_vector_type(2)));

// four int8 (one dword, k ascending from the low byte) -> two dwords of
// packed bf16 pairs (k, k+1) and (k+2, k+3), low half = lower k: the layout
// of the bf16 x pairs they meet in v_dot2
DEVINL void cvt4_i8_bf16(unsigned int w, unsigned int& p01,
                         unsigned int& p23) {
  const float f0 = (float)(int)(signed char)(w & 0xffu);
  const float f1 = (float)(int)(signed char)((w >> 8) & 0xffu);
  const float f2 = (float)(int)(signed char)((w >> 16) & 0xffu);
  const float f3 = (float)((int)w >> 24);
  // exact (see above), so the rounding mode of the pack does not matter;
  // written as a vector convert so that it is ONE v_cvt_pk_bf16_f32 per pair
  union { bf2_i8 v; unsigned int u; } a, b;
  a.v = __builtin_convertvector(f2_i8{f0, f1}, bf2_i8);
  b.v = __builtin_convertvector(f2_i8{f2, f3}, bf2_i8);
  p01 = a.u;
  p23 = b.u;
}

DEVINL void cvt16_i8_bf16(const uint4& w, unsigned int (&p)[8]) {
  cvt4_i8_bf16(w.x, p[0], p[1]);
  cvt4_i8_bf16(w.y, p[2], p[3]);
  cvt4_i8_bf16(w.z, p[4], p[5]);
  cvt4_i8_bf16(w.w, p[6], p[7]);
}

DEVINL sv2_i8 as_sv2(unsigned int u) {
  union { unsigned int u; sv2_i8 v; } c;
  c.u = u;
  return c.v;
}

template <int MT, int R>
__global__ __launch_bounds__(GEMV8_BLOCK) void gemv_w8a16_kernel(
    const ushort* __restrict__ x, const signed char* __restrict__ q,
    const float* __restrict__ scale, const ushort* __restrict__ bias,
    ushort* __restrict__ y, int M, long N, long K, int has_bias) {
  // the bf16 kernel's x tile, so LDS (and with it occupancy) is unchanged
  constexpr int KT = (MT <= 16) ? 2048 : 1024;
  constexpr int NCH = KT / GEMV8_WSTEP;  // 16-byte chunks per lane and row
  __shared__ ushort xs[MT * KT];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long n0 = ((long)blockIdx.x * 4 + wave) * R;
  const bool live = n0 < N;
  float acc[R][MT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

  for (long k0 = 0; k0 < K; k0 += KT) {
    const int kt = (int)min((long)KT, K - k0);
    // the tile's weights first: they are in flight while x is staged
    uint4 w[R][NCH];
    if (live) {
      const signed char* q0 = q + n0 * K + k0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        // a row past N re-reads row n0; its sums are never stored
        const signed char* qr = (n0 + r < N) ? q0 + r * K : q0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int kk = c * GEMV8_WSTEP + lane * 16;
          // kt is a multiple of 16: the whole chunk is inside
          if (kk < kt) w[r][c] = *(const uint4*)&qr[kk];
        }
      }
    }
    // cooperative x stage (vectorized 16 B; kt is a multiple of 8)
    for (int i = threadIdx.x * 8; i < M * kt; i += GEMV8_BLOCK * 8) {
      const int m = i / kt, c = i % kt;
      *(uint4*)&xs[m * KT + c] = *(const uint4*)&x[(long)m * K + k0 + c];
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int kk = c * GEMV8_WSTEP + lane * 16;
        if (kk < kt) {
          unsigned int p[R][8];
#pragma unroll
          for (int r = 0; r < R; ++r) cvt16_i8_bf16(w[r][c], p[r]);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            if (m < M) {
              const uint4 xlo = *(const uint4*)&xs[m * KT + kk];
              const uint4 xhi = *(const uint4*)&xs[m * KT + kk + 8];
              const unsigned int xv[8] = {xlo.x, xlo.y, xlo.z, xlo.w,
                                          xhi.x, xhi.y, xhi.z, xhi.w};
#pragma unroll
              for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < R; ++r)
                  acc[r][m] = __builtin_amdgcn_fdot2_f32_bf16(
                      as_sv2(p[r][j]), as_sv2(xv[j]), acc[r][m], false);
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
        const float s = scale[n0 + r];
        const float b = has_bias ? bf2f(bias[n0 + r]) : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < M) y[(long)m * N + n0 + r] = f2bf(s * acc[r][m] + b);
      }
    }
  }
}

// Rows per wave.  2 keeps the bf16 kernel's grid (N / 8 workgroups) and its
// occupancy for every MT.  R = 4 compiles without scratch and would halve the
// x bytes each workgroup re-stages and the LDS reads per weight, but its
// registers cost occupancy (waves/SIMD 5/4/4/4/2/1 for MT 1..32 against the
// bf16 kernel's 8/8/8/5/2/2), so it is not instantiated.
#define GEMV8_ROWS 2

torch::Tensor gemv_w8a16(torch::Tensor x, torch::Tensor q,
                         torch::Tensor scale,
                         c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(x.is_cuda() && q.is_cuda() && scale.is_cuda(),
              "gemv_w8a16: device tensors only");
  TORCH_CHECK(x.is_contiguous() && q.is_contiguous() &&
              scale.is_contiguous(), "gemv_w8a16: contiguous operands only");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "gemv_w8a16: x is bf16");
  TORCH_CHECK(q.scalar_type() == torch::kChar, "gemv_w8a16: q is int8");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat,
              "gemv_w8a16: scale is fp32");
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && x.size(1) == q.size(1),
              "gemv_w8a16: x (M,K) and q (N,K)");
  const int M = (int)x.size(0);
  const long N = q.size(0), K = q.size(1);
  TORCH_CHECK(scale.numel() == N, "gemv_w8a16: one scale per output row");
  TORCH_CHECK(M >= 1 && M <= 32, "gemv_w8a16 is the M<=32 decode path");
  TORCH_CHECK(N >= 1 && K >= 16 && K % 16 == 0,
              "gemv_w8a16: K must be a multiple of 16");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
              (uintptr_t)q.data_ptr() % 16 == 0,
              "gemv_w8a16: x and q must be 16-byte aligned");
  const ushort* bptr = nullptr;
  int has_bias = 0;
  if (bias.has_value() && bias->numel() > 0) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                bias->scalar_type() == torch::kBFloat16 &&
                bias->numel() == N,
                "gemv_w8a16: bias is contiguous bf16 with N elements");
    bptr = (const ushort*)bias->data_ptr();
    has_bias = 1;
  }
  auto y = torch::empty({M, N}, x.options());
  constexpr int R = GEMV8_ROWS;
  const dim3 grid((unsigned)((N + 4 * R - 1) / (4 * R))), block(GEMV8_BLOCK);
  auto stream = at::cuda::getCurrentHIPStream();
  const ushort* xp = (const ushort*)x.data_ptr();
  const signed char* qp = (const signed char*)q.data_ptr();
  const float* sp = (const float*)scale.data_ptr();
  ushort* yp = (ushort*)y.data_ptr();
#define LAUNCH(MT_)                                                       \
  hipLaunchKernelGGL((gemv_w8a16_kernel<MT_, R>), grid, block, 0, stream, \
                     xp, qp, sp, bptr, yp, M, N, K, has_bias)
  if (M == 1) LAUNCH(1);
  else if (M == 2) LAUNCH(2);
  else if (M <= 4) LAUNCH(4);
  else if (M <= 8) LAUNCH(8);
  else if (M <= 16) LAUNCH(16);
  else LAUNCH(32);
#undef LAUNCH
  TORCH_CHECK(hipGetLastError() == hipSuccess);
  return y;
}
