// fp8 (OCP e4m3) KV cache: quantising append and dequantise.
//
// A cache row is one (batch, kv head, position): D bytes of e4m3 in a uint8
// tensor (B, Hkv, Smax, D) plus one fp32 scale in a tensor (B, Hkv, Smax).
// The scale is a power of two chosen per row when the row is written:
//   amax = max|x| = m * 2^e, m in [0.5, 1)
//   scale = 2^(e-9) if m <= 0.875 else 2^(e-8), exponent floored at -64
// so amax/scale lies in (224, 448] (448 = 0.875 * 2^9 is the e4m3 maximum)
// and x/scale, a bf16 value times a power of two, is exact in fp32.  The
// stored byte is e4m3_rne(x/scale); |x/scale| <= 448 by construction, so the
// converter's overflow behaviour is never met.  Non-finite inputs are out of
// contract.  ops/kv_fp8.py holds the same rule in torch (the oracle).
//
// Append (one launch for K and V): D/8 lanes own a row.  Each lane loads 16
// bytes of bf16, the row's amax comes from a DPP max over the lane group,
// the scale from amax's exponent bits, and eight values go through
// v_cvt_pk_fp8_f32 into two dwords and one 8-byte store; lane 0 of the group
// stores the scale.  The position is a kernel argument or is read from an
// int64 device tensor (1 or B elements), clamped to [0, Smax-S] before any
// address is formed, so the launch captures into a hipGraph.
//
// Dequantise: elementwise, 8 bytes per thread through v_cvt_pk_f32_fp8,
// times the row scale, written as bf16 or fp32 (both exact).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "decode_attn_common.h"

// no packed-fp32 VALU forms in this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

#define KVQ_BLOCK 256
#define KVQ_EXP_FLOOR (127 - 64)   // biased exponent of the smallest scale

typedef float kvq_fv2 __attribute__((ext_vector_type(2)));

template <int CTRL>
DEVINL float kvq_dpp_max(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF,
                                            0xF, false);
  return fmaxf(v, __int_as_float(t));
}

// all-reduce max over aligned groups of LPR (8 or 16) lanes
template <int LPR>
DEVINL float kvq_group_max(float v) {
  if (LPR == 16) v = kvq_dpp_max<0x140>(v);  // row_mirror
  v = kvq_dpp_max<0x141>(v);                 // row_half_mirror
  v = kvq_dpp_max<0xB1>(v);                  // quad_perm [1,0,3,2]
  v = kvq_dpp_max<0x4E>(v);                  // quad_perm [2,3,0,1]
  return v;
}

// rows are numbered (kv, b, h, s): kv = 0 takes k into the K cache, 1 takes
// v into the V cache
template <int D>
__global__ __launch_bounds__(KVQ_BLOCK) void kv_fp8_append_kernel(
    const ushort* __restrict__ k, const ushort* __restrict__ v,
    uint8_t* __restrict__ kd, float* __restrict__ ks,
    uint8_t* __restrict__ vd, float* __restrict__ vs,
    const long* __restrict__ pos_ptr, int pos_stride, long pos_host, int B,
    int Hkv, int S, int Smax, long k_sb, long k_sh, long k_ss, long v_sb,
    long v_sh, long v_ss) {
  constexpr int LPR = D / 8;                 // lanes per row
  constexpr int RPB = KVQ_BLOCK / LPR;       // rows per block
  const long nrow = (long)B * Hkv * S;       // per tensor
  const long r_raw = (long)blockIdx.x * RPB + threadIdx.x / LPR;
  const bool live = r_raw < 2 * nrow;
  // a lane past the end redoes the last row and stores nothing: every lane
  // of a group stays in the DPP reduction
  const long r = live ? r_raw : 2 * nrow - 1;
  const int ld = threadIdx.x % LPR;
  const bool is_v = r >= nrow;
  const long rr = is_v ? r - nrow : r;
  const int s = (int)(rr % S);
  const int h = (int)((rr / S) % Hkv);
  const int b = (int)(rr / ((long)S * Hkv));
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, S);

  const ushort* src = is_v ? v + (long)b * v_sb + (long)h * v_sh + (long)s * v_ss
                           : k + (long)b * k_sb + (long)h * k_sh + (long)s * k_ss;
  const uint4 raw = *(const uint4*)&src[ld * 8];
  const uint* w = (const uint*)&raw;
  float x[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[2 * e] = __uint_as_float(w[e] << 16);
    x[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
  }
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[e]));
  amax = kvq_group_max<LPR>(amax);

  // amax = 1.f * 2^(E-127) = m * 2^(E-126) with m = 1.f / 2:
  // m <= 0.875 <=> mantissa field <= 0x600000; scale exponent e-9 or e-8
  const uint ab = __float_as_uint(amax);
  int se = (int)(ab >> 23) - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
  se = max(se, KVQ_EXP_FLOOR);               // also the all-zero row
  const float scale = __uint_as_float((uint)se << 23);
  const float inv = __uint_as_float((uint)(254 - se) << 23);

  uint2 pk;
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
  pk.x = (uint)lo;
  pk.y = (uint)hi;
  if (!live) return;
  const long row = ((long)b * Hkv + h) * Smax + p0 + s;
  uint8_t* dd = is_v ? vd : kd;
  float* ds = is_v ? vs : ks;
  *(uint2*)&dd[row * D + ld * 8] = pk;
  if (ld == 0) ds[row] = scale;
}

// out (BH, L, D) dense <- data (BH, Smax, D), scale (BH, Smax); 8 elements
// per thread
template <bool BF16>
__global__ __launch_bounds__(KVQ_BLOCK) void kv_fp8_dequant_kernel(
    const uint8_t* __restrict__ data, const float* __restrict__ scale,
    void* __restrict__ out, long n8, int L, int Smax, int D) {
  const long i = (long)blockIdx.x * KVQ_BLOCK + threadIdx.x;
  if (i >= n8) return;
  const int d8 = D / 8;
  const long orow = i / d8;                  // bh * L + l
  const int c = (int)(i % d8);
  const long srow = (orow / L) * Smax + orow % L;
  const uint2 pk = *(const uint2*)&data[srow * D + c * 8];
  const float sc = scale[srow];
  float f[8];
  const kvq_fv2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)pk.x, false);
  const kvq_fv2 a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)pk.x, true);
  const kvq_fv2 a2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)pk.y, false);
  const kvq_fv2 a3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)pk.y, true);
  f[0] = a0.x * sc; f[1] = a0.y * sc; f[2] = a1.x * sc; f[3] = a1.y * sc;
  f[4] = a2.x * sc; f[5] = a2.y * sc; f[6] = a3.x * sc; f[7] = a3.y * sc;
  if (BF16) {
    // e4m3 times a power of two is exact in bf16: the high half is the value
    uint4 o;
    uint* ow = (uint*)&o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      ow[e] = (__float_as_uint(f[2 * e]) >> 16) |
              (__float_as_uint(f[2 * e + 1]) & 0xffff0000u);
    *(uint4*)((ushort*)out + orow * D + c * 8) = o;
  } else {
    float* op = (float*)out + orow * D + c * 8;
    *(float4*)op = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(op + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

#pragma clang attribute pop

static void kvq_check_cache(const torch::Tensor& data,
                            const torch::Tensor& scale, const char* name) {
  TORCH_CHECK(data.is_cuda() && data.scalar_type() == torch::kByte &&
                  data.dim() == 4 && data.is_contiguous(),
              "fp8 kv cache: ", name, ".data must be contiguous 4-D uint8 CUDA");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat &&
                  scale.dim() == 3 && scale.is_contiguous() &&
                  scale.size(0) == data.size(0) &&
                  scale.size(1) == data.size(1) &&
                  scale.size(2) == data.size(2),
              "fp8 kv cache: ", name,
              ".scale must be contiguous fp32 (B, Hkv, Smax)");
  TORCH_CHECK(((uintptr_t)data.data_ptr()) % 16 == 0 && data.size(3) % 8 == 0,
              "fp8 kv cache: ", name, ".data must allow 8-byte accesses");
}

static void kvq_check_src(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 4 && t.stride(3) == 1,
              "kv_cache_append: ", name,
              " must be 4-D bf16 CUDA with contiguous head dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr()) % 16 == 0,
              "kv_cache_append: ", name,
              " must allow 16-byte loads (strides % 8, 16-byte base)");
}

// k, v (B, Hkv, S, D) bf16 -> rows [pos, pos+S) of both caches, one launch.
// pos_t: optional int64 device tensor (1 or B elements) that overrides pos0.
void kv_fp8_append(torch::Tensor k_data, torch::Tensor k_scale,
                   torch::Tensor v_data, torch::Tensor v_scale,
                   torch::Tensor k, torch::Tensor v,
                   c10::optional<torch::Tensor> pos_t, long pos0) {
  kvq_check_cache(k_data, k_scale, "k_cache");
  kvq_check_cache(v_data, v_scale, "v_cache");
  kvq_check_src(k, "k");
  kvq_check_src(v, "v");
  const int B = k.size(0), Hkv = k.size(1), D = k.size(3);
  const long S = k.size(2), Smax = k_data.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "kv_cache_append: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(v.sizes() == k.sizes() && v_data.sizes() == k_data.sizes(),
              "kv_cache_append: k/v shape mismatch");
  TORCH_CHECK(k_data.size(0) == B && k_data.size(1) == Hkv &&
                  k_data.size(3) == D,
              "kv_cache_append: cache shape mismatch");
  TORCH_CHECK(S >= 1 && S <= Smax && Smax < (1L << 30));
  const long* pos_ptr = nullptr;
  int pos_stride = 0;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->is_cuda() && pos_t->scalar_type() == torch::kLong &&
                    pos_t->is_contiguous() &&
                    (pos_t->numel() == 1 || pos_t->numel() == B),
                "kv_cache_append: pos0 tensor must be int64 CUDA with 1 or "
                "B elements");
    pos_ptr = (const long*)pos_t->data_ptr();
    pos_stride = pos_t->numel() == 1 ? 0 : 1;
  } else {
    TORCH_CHECK(pos0 >= 0 && pos0 + S <= Smax, "kv_cache_append: pos0=", pos0,
                " with S=", S, " outside the cache (Smax=", Smax, ")");
  }
  const long rows = 2L * B * Hkv * S;
  const int rpb = KVQ_BLOCK / (D / 8);
  const long nblk = (rows + rpb - 1) / rpb;
  TORCH_CHECK(nblk < (1L << 31));
  auto stream = at::cuda::getCurrentHIPStream();
#define KVQ_APPEND(D_)                                                       \
  hipLaunchKernelGGL((kv_fp8_append_kernel<D_>), dim3((unsigned)nblk),       \
                     dim3(KVQ_BLOCK), 0, stream,                             \
                     (const ushort*)k.data_ptr(), (const ushort*)v.data_ptr(), \
                     k_data.data_ptr<uint8_t>(), k_scale.data_ptr<float>(),  \
                     v_data.data_ptr<uint8_t>(), v_scale.data_ptr<float>(),  \
                     pos_ptr, pos_stride, pos0, B, Hkv, (int)S, (int)Smax,   \
                     k.stride(0), k.stride(1), k.stride(2), v.stride(0),     \
                     v.stride(1), v.stride(2))
  if (D == 64) KVQ_APPEND(64); else KVQ_APPEND(128);
#undef KVQ_APPEND
  HIP_CHECK_LAST();
}

// dense (B, Hkv, length, D) bf16 or fp32 from the first `length` positions
torch::Tensor kv_fp8_dequant(torch::Tensor data, torch::Tensor scale,
                             long length, bool to_bf16) {
  kvq_check_cache(data, scale, "cache");
  const long B = data.size(0), Hkv = data.size(1), Smax = data.size(2),
             D = data.size(3);
  TORCH_CHECK(length >= 0 && length <= Smax && Smax < (1L << 30),
              "Fp8KV.dequantize: length ", length, " outside the cache");
  auto out = torch::empty(
      {B, Hkv, length, D},
      data.options().dtype(to_bf16 ? torch::kBFloat16 : torch::kFloat));
  const long n8 = B * Hkv * length * (D / 8);
  if (n8 == 0) return out;
  const long nblk = (n8 + KVQ_BLOCK - 1) / KVQ_BLOCK;
  TORCH_CHECK(nblk < (1L << 31));
  auto stream = at::cuda::getCurrentHIPStream();
  if (to_bf16)
    hipLaunchKernelGGL((kv_fp8_dequant_kernel<true>), dim3((unsigned)nblk),
                       dim3(KVQ_BLOCK), 0, stream, data.data_ptr<uint8_t>(),
                       scale.data_ptr<float>(), out.data_ptr(), n8,
                       (int)length, (int)Smax, (int)D);
  else
    hipLaunchKernelGGL((kv_fp8_dequant_kernel<false>), dim3((unsigned)nblk),
                       dim3(KVQ_BLOCK), 0, stream, data.data_ptr<uint8_t>(),
                       scale.data_ptr<float>(), out.data_ptr(), n8,
                       (int)length, (int)Smax, (int)D);
  HIP_CHECK_LAST();
  return out;
}
