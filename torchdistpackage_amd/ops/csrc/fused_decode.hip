// Fused glue kernels of the Llama single-token decode step.
//
// One decode_step used to launch 18 kernels per layer, seven of them moving a
// few KB each: rope(q), rope(k), two cache writes, two residual adds and the
// SwiGLU.  Three kernels fold them into their neighbours:
//
//   gemv_swiglu_bf16      silu(x @ Wg^T) * (x @ Wu^T): the gate and up GEMVs
//                         and the SwiGLU in one launch
//   rope_kv_append_kernel RoPE on q and k, rotated k and v into the dense
//                         caches: one launch instead of four
//   add_rmsnorm_kernel    x_new = x + y and h = rms_norm(x_new): the residual
//                         add folded into the norm that follows it
//
// Each one makes exactly the roundings of the kernels it replaces (gemv.hip,
// rope_swiglu.hip, norms.hip and torch's bf16 add), in the same order, so its
// results are theirs bit for bit; the expressions below are kept in the form
// those files use for that reason.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "fused_checks.h"

namespace {

constexpr int BLOCK = 256;

typedef short sv2 __attribute__((ext_vector_type(2)));

// as swiglu_fwd_kernel (rope_swiglu.hip)
DEVINL float sigmoidf_fast(float x) {
  return 1.0f / (1.0f + __builtin_exp2f(-1.442695041f * x));
}

DEVINL void unpack8(const uint4& u, float* f) {
  const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = bf2f((unsigned short)(w[j] & 0xffffu));
    f[2 * j + 1] = bf2f((unsigned short)(w[j] >> 16));
  }
}

DEVINL uint4 pack8(const float* f) {
  unsigned int w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = (unsigned int)f2bf(f[2 * j]) |
           ((unsigned int)f2bf(f[2 * j + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------- gate/up GEMV+SwiGLU
//
// The streaming design of gemv_bf16_kernel: x staged once per workgroup
// through LDS in KT-wide tiles, weights read 16 bytes per lane, fp32
// accumulation by v_dot2_f32_bf16, a wave owns two weight rows.  Here the two
// rows are row n of Wg and row n of Wu, so after the wave reduction lane 0
// holds both operands of silu(a) * b for column n and the (M, N) gate and up
// outputs never reach memory.  4 waves = 4 columns per workgroup; the bytes
// in flight per lane are those of gemv_bf16_kernel.
template <int MT>
__global__ __launch_bounds__(BLOCK) void gemv_swiglu_bf16(
    const ushort* __restrict__ x, const ushort* __restrict__ Wg,
    const ushort* __restrict__ Wu, ushort* __restrict__ y, int M, long N,
    long K) {
  constexpr int KT = 2048;                 // LDS x tile: MT*KT*2 <= 32 KB
  __shared__ ushort xs[MT * KT];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + wave;
  float acc0[MT], acc1[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc0[m] = acc1[m] = 0.f;

  for (long k0 = 0; k0 < K; k0 += KT) {
    const int kt = (int)min((long)KT, K - k0);
    // cooperative x stage (vectorized 16 B; kt is a multiple of 8)
    for (int i = threadIdx.x * 8; i < M * kt; i += BLOCK * 8) {
      const int m = i / kt, c = i % kt;
      *(uint4*)&xs[m * KT + c] = *(const uint4*)&x[(long)m * K + k0 + c];
    }
    __syncthreads();
    if (n < N) {
      const ushort* w0 = Wg + n * K + k0;
      const ushort* w1 = Wu + n * K + k0;
      for (int kk = lane * 8; kk < kt; kk += WAVE * 8) {
        const uint4 wa = *(const uint4*)&w0[kk];
        const uint4 wb = *(const uint4*)&w1[kk];
        const sv2* wpa = (const sv2*)&wa;
        const sv2* wpb = (const sv2*)&wb;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m < M) {
            const uint4 xv = *(const uint4*)&xs[m * KT + kk];
            const sv2* xp = (const sv2*)&xv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc0[m] = __builtin_amdgcn_fdot2_f32_bf16(wpa[j], xp[j],
                                                        acc0[m], false);
              acc1[m] = __builtin_amdgcn_fdot2_f32_bf16(wpb[j], xp[j],
                                                        acc1[m], false);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (n >= N) return;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc0[m] = wave_sum(acc0[m]);
    acc1[m] = wave_sum(acc1[m]);
  }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < M) {
        // the roundings of the two unfused GEMVs, then swiglu_fwd_kernel
        const float a = bf2f(f2bf(acc0[m]));
        const float b = bf2f(f2bf(acc1[m]));
        y[(long)m * N + n] = f2bf(a * sigmoidf_fast(a) * b);
      }
  }
}

// ------------------------------------------------------ RoPE + cache append
//
// One flat grid over the B * (H + 2 * Hkv) * S rows: q rows first, then k,
// then v.  A lane owns the 8 elements at c and the 8 at c + D/2 of one row
// (two 16-byte loads, two 16-byte stores): for q and k that is the rotate-half
// pair of rope_kernel<true>, for v a copy.  With D = 128 a wave covers 8
// rows, so the row kind is wave-uniform whenever the q and k row counts are
// multiples of 8 (of 16 at D = 64).
struct RkaArgs {
  const unsigned short* src[3];     // q, k, v: (B, heads, S, D), D contiguous
  unsigned short* dst[3];           // q out (contiguous), k cache, v cache
  long ss[3][3];                    // source strides over (b, head, s)
  long ds[3][3];                    // destination strides over (b, head, s)
  const float* cs;                  // (rows, D/2) cos
  const float* sn;                  // (rows, D/2) sin
  const long* pos0p;                // device position, or null
  long q_rows, kv_rows;             // B*H*S, B*Hkv*S
  int H, Hkv, S, D, pos0, pos_max;
};

__global__ __launch_bounds__(BLOCK) void rope_kv_append_kernel(RkaArgs a) {
  const int half = a.D >> 1;
  const int chunks = half >> 3;
  const long total = (a.q_rows + 2 * a.kv_rows) * chunks;
  // a device position is bounded by nothing on the host: clamp it to
  // [0, pos_max] (pos_max = min(table rows, Smax) - S) before any address is
  // formed, as rope_kernel and da_read_pos do
  int p0 = a.pos0;
  if (a.pos0p) {
    const long p = *a.pos0p;
    p0 = (int)(p < 0 ? 0 : (p > (long)a.pos_max ? (long)a.pos_max : p));
  }
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (long)gridDim.x * blockDim.x) {
    const long row = g / chunks;
    const int c = (int)(g - row * chunks) * 8;
    const int kind = row < a.q_rows ? 0 : (row < a.q_rows + a.kv_rows ? 1 : 2);
    const long r = row - (kind == 0 ? 0 : a.q_rows + (kind - 1) * a.kv_rows);
    const long heads = kind == 0 ? a.H : a.Hkv;
    const long bh = r / a.S;
    const int s = (int)(r - bh * a.S);
    const long b = bh / heads, h = bh - b * heads;
    const unsigned short* sp = a.src[kind] + b * a.ss[kind][0] +
                               h * a.ss[kind][1] + s * a.ss[kind][2] + c;
    // q keeps its own row index; the caches are written at p0 + s
    unsigned short* dp = a.dst[kind] + b * a.ds[kind][0] + h * a.ds[kind][1] +
                         (long)(kind == 0 ? s : p0 + s) * a.ds[kind][2] + c;
    const uint4 u1 = *(const uint4*)sp;
    const uint4 u2 = *(const uint4*)(sp + half);
    if (kind == 2) {
      *(uint4*)dp = u1;
      *(uint4*)(dp + half) = u2;
      continue;
    }
    float x1[8], x2[8], co[8], si[8];
    unpack8(u1, x1);
    unpack8(u2, x2);
    const long t = (long)(p0 + s) * half + c;
#pragma unroll
    for (int j = 0; j < 8; j += 4) {
      *(float4*)(co + j) = *(const float4*)(a.cs + t + j);
      *(float4*)(si + j) = *(const float4*)(a.sn + t + j);
    }
    float y1[8], y2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y1[j] = x1[j] * co[j] - x2[j] * si[j];
      y2[j] = x2[j] * co[j] + x1[j] * si[j];
    }
    *(uint4*)dp = pack8(y1);
    *(uint4*)(dp + half) = pack8(y2);
  }
}

// ----------------------------------------------------- residual add + RMSNorm
//
// rmsnorm_fwd_bf16v8 (norms.hip) with the residual add in front: one
// workgroup per row; the first sweep forms x_new = bf16(x + y), stores it and
// sums the squares of the ROUNDED values in that kernel's element-to-thread
// assignment and block_sum order; the second sweep scales them.  NC > 0 keeps
// a thread's NC chunks of x_new packed in registers between the sweeps
// (D <= NC * 2048); NC == 0 re-reads the thread's own stores.
template <int NC>
__global__ __launch_bounds__(BLOCK) void add_rmsnorm_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ y,
    const unsigned short* __restrict__ w, unsigned short* __restrict__ xn,
    unsigned short* __restrict__ h, int rows, int D, float eps) {
  __shared__ float lds[BLOCK / WAVE];
  constexpr int NR = NC > 0 ? NC : 1;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* xr = x + (long)row * D;
    const unsigned short* yr = y + (long)row * D;
    unsigned short* nr = xn + (long)row * D;
    unsigned short* hr = h + (long)row * D;
    uint4 keep[NR];
    float ss = 0.f;
    auto first = [&](int i) -> uint4 {
      float a[8], b[8], v[8];
      unpack8(*(const uint4*)(xr + i), a);
      unpack8(*(const uint4*)(yr + i), b);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a[j] + b[j];
      const uint4 p = pack8(v);
      *(uint4*)(nr + i) = p;
      unpack8(p, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
      return p;
    };
    if (NC > 0) {
#pragma unroll
      for (int c = 0; c < NR; ++c) {
        const int i = threadIdx.x * 8 + c * BLOCK * 8;
        if (i < D) keep[c] = first(i);
      }
    } else {
      for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) first(i);
    }
    ss = block_sum<BLOCK>(ss, lds);
    float r = rsqrtf(ss / D + eps);
    auto second = [&](int i, const uint4& p) {
      float v[8], wv[8], out[8];
      unpack8(p, v);
      unpack8(*(const uint4*)(w + i), wv);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = v[j] * r * wv[j];
      *(uint4*)(hr + i) = pack8(out);
    };
    if (NC > 0) {
#pragma unroll
      for (int c = 0; c < NR; ++c) {
        const int i = threadIdx.x * 8 + c * BLOCK * 8;
        if (i < D) second(i, keep[c]);
      }
    } else {
      // a thread reads back only what it stored itself
      for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8)
        second(i, *(const uint4*)(nr + i));
    }
    __syncthreads();
  }
}

}  // namespace

// ------------------------------------------------------------------ C++ API

// x (M, K), w_gate / w_up (N, K), all contiguous bf16 -> (M, N) bf16
torch::Tensor gemv_swiglu(torch::Tensor x, torch::Tensor w_gate,
                          torch::Tensor w_up) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                  x.scalar_type() == torch::kBFloat16 && aligned16(x),
              "gemv_swiglu: x must be a contiguous 16-byte aligned (M, K) "
              "bf16 CUDA tensor");
  TORCH_CHECK(w_gate.dim() == 2 && w_gate.size(1) == x.size(1),
              "gemv_swiglu: w_gate must be (N, K) with x's K");
  check_bf16_rows("gemv_swiglu", "w_gate", w_gate, w_gate);
  check_bf16_rows("gemv_swiglu", "w_up", w_up, w_gate);
  TORCH_CHECK(w_gate.device() == x.device(),
              "gemv_swiglu: weights must be on x's device");
  const int M = (int)x.size(0);
  const long N = w_gate.size(0), K = w_gate.size(1);
  TORCH_CHECK(M >= 1 && M <= 8, "gemv_swiglu is the M <= 8 decode path");
  TORCH_CHECK(K % 8 == 0 && K > 0, "K must be a positive multiple of 8");
  auto y = torch::empty({M, N}, x.options());
  if (N == 0) return y;
  const dim3 grid((unsigned)((N + 3) / 4)), block(BLOCK);
  auto stream = at::cuda::getCurrentHIPStream();
  const ushort* xp = (const ushort*)x.data_ptr();
  const ushort* gp = (const ushort*)w_gate.data_ptr();
  const ushort* up = (const ushort*)w_up.data_ptr();
  ushort* yp = (ushort*)y.data_ptr();
#define LAUNCH(MT_)                                                       \
  hipLaunchKernelGGL((gemv_swiglu_bf16<MT_>), grid, block, 0, stream, xp, \
                     gp, up, yp, M, N, K)
  if (M == 1) LAUNCH(1);
  else if (M == 2) LAUNCH(2);
  else if (M <= 4) LAUNCH(4);
  else LAUNCH(8);
#undef LAUNCH
  HIP_CHECK_LAST();
  return y;
}

// q (B, H, S, D), k / v (B, Hkv, S, D): bf16, D contiguous; caches
// (B, Hkv, Smax, D) bf16, D contiguous; cos / sin (rows, D/2) fp32.  Returns
// rotated q, contiguous; writes rotated k and v at [pos, pos + S).
torch::Tensor rope_kv_append(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                             torch::Tensor cs, torch::Tensor sn,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             c10::optional<torch::Tensor> pos_t, long pos0) {
  const char* fn = "rope_kv_append";
  TORCH_CHECK(q.is_cuda() && q.dim() == 4, fn, ": q must be 4-D on the GPU");
  const long B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, fn, ": head dim 64 or 128, got ", D);
  TORCH_CHECK(k.dim() == 4 && v.sizes() == k.sizes() && k.size(0) == B &&
                  k.size(2) == S && k.size(3) == D,
              fn, ": k and v must be (B, Hkv, S, D) with q's B, S and D");
  const long Hkv = k.size(1);
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
                  k_cache.size(0) == B && k_cache.size(1) == Hkv &&
                  k_cache.size(3) == D,
              fn, ": the caches must both be (B, Hkv, Smax, D)");
  const long Smax = k_cache.size(2);
  // 16-byte accesses at c and c + D/2 of every row: the base pointers and
  // every stride that gets multiplied by a non-zero index must keep them
  // aligned
  auto ok = [&](const torch::Tensor& t) {
    bool r = t.is_cuda() && t.device() == q.device() &&
             t.scalar_type() == torch::kBFloat16 && t.stride(3) == 1 &&
             aligned16(t);
    for (int d = 0; d < 3; ++d)
      r = r && (t.size(d) <= 1 || t.stride(d) % 8 == 0);
    return r;
  };
  TORCH_CHECK(ok(q) && ok(k) && ok(v) && ok(k_cache) && ok(v_cache), fn,
              ": q, k, v and the caches must be bf16 on one GPU with a "
              "contiguous head dim, strides that are multiples of 8 elements "
              "and 16-byte aligned base pointers");
  TORCH_CHECK(cs.device() == q.device() && sn.device() == q.device() &&
                  cs.scalar_type() == torch::kFloat &&
                  sn.scalar_type() == torch::kFloat && cs.dim() == 2 &&
                  cs.is_contiguous() && sn.is_contiguous() &&
                  sn.sizes() == cs.sizes() && cs.size(1) == D / 2 &&
                  aligned16(cs) && aligned16(sn),
              fn, ": cos / sin must be contiguous 16-byte aligned "
              "(rows, D/2) fp32 tables on q's device");
  const long lim = std::min((long)cs.size(0), Smax);
  TORCH_CHECK(S >= 1 && S <= lim, fn, ": S=", S, " exceeds the cos/sin table "
              "or the cache (", cs.size(0), " rows, Smax=", Smax, ")");
  const long* pp = nullptr;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->device() == q.device() &&
                    pos_t->scalar_type() == torch::kLong &&
                    pos_t->numel() == 1,
                fn, ": pos must be a 1-element int64 tensor on q's device");
    pp = (const long*)pos_t->data_ptr();
    pos0 = 0;
  } else {
    TORCH_CHECK(pos0 >= 0 && pos0 + S <= lim, fn, ": pos0=", pos0, " with S=",
                S, " outside the cos/sin table or the cache (", cs.size(0),
                " rows, Smax=", Smax, ")");
  }
  auto qo = torch::empty({B, H, S, D}, q.options());
  RkaArgs a;
  const torch::Tensor* src[3] = {&q, &k, &v};
  const torch::Tensor* dst[3] = {&qo, &k_cache, &v_cache};
  for (int i = 0; i < 3; ++i) {
    a.src[i] = (const unsigned short*)src[i]->data_ptr();
    a.dst[i] = (unsigned short*)dst[i]->data_ptr();
    for (int d = 0; d < 3; ++d) {
      a.ss[i][d] = src[i]->stride(d);
      a.ds[i][d] = dst[i]->stride(d);
    }
  }
  a.cs = cs.data_ptr<float>();
  a.sn = sn.data_ptr<float>();
  a.pos0p = pp;
  a.q_rows = B * H * S;
  a.kv_rows = B * Hkv * S;
  a.H = (int)H; a.Hkv = (int)Hkv; a.S = (int)S; a.D = (int)D;
  a.pos0 = (int)pos0;
  a.pos_max = (int)(lim - S);
  const long total = (a.q_rows + 2 * a.kv_rows) * (D / 16);
  if (total == 0) return qo;
  const long nb = (total + BLOCK - 1) / BLOCK;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(rope_kv_append_kernel,
                     dim3((unsigned)std::min(nb, (long)65535 * 8)),
                     dim3(BLOCK), 0, stream, a);
  HIP_CHECK_LAST();
  return qo;
}

// x, y (..., D) bf16, w (D,) bf16 -> (bf16(x + y), rms_norm of that)
std::vector<torch::Tensor> add_rmsnorm(torch::Tensor x, torch::Tensor y,
                                       torch::Tensor w, double eps) {
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "add_rmsnorm: empty x");
  const int D = (int)x.size(-1);
  TORCH_CHECK(D % 8 == 0 && D <= 16384,
              "add_rmsnorm: D must be a multiple of 8, at most 16384");
  check_bf16_rows("add_rmsnorm", "x", x, x);
  check_bf16_rows("add_rmsnorm", "y", y, x);
  check_bf16_vec("add_rmsnorm", "weight", w, x, D);
  const long rows = x.numel() / D;
  auto xn = torch::empty_like(x);
  auto h = torch::empty_like(x);
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid((unsigned)std::min(rows, 2048L)), block(BLOCK);
  const int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define LAUNCH(NC_)                                                        \
  hipLaunchKernelGGL((add_rmsnorm_kernel<NC_>), grid, block, 0, stream,    \
                     (const unsigned short*)x.data_ptr(),                  \
                     (const unsigned short*)y.data_ptr(),                  \
                     (const unsigned short*)w.data_ptr(),                  \
                     (unsigned short*)xn.data_ptr(),                       \
                     (unsigned short*)h.data_ptr(), (int)rows, D, (float)eps)
  if (nc == 1) LAUNCH(1);
  else if (nc == 2) LAUNCH(2);
  else if (nc == 3) LAUNCH(3);
  else if (nc == 4) LAUNCH(4);
  else LAUNCH(0);
#undef LAUNCH
  HIP_CHECK_LAST();
  return {xn, h};
}
