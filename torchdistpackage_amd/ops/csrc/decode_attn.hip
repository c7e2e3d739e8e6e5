// Split-KV decode attention over a KV cache (flash-decoding), bf16, hd 64/128.
//
// q (B, Hq, Sq, D) attends to k/v caches (B, Hkv, Smax, D); query row i sees
// cache positions [0, pos0+i].  Decode attention is a memory-bound read of
// K and V, so the design is a pure stream:
//  - grid (B*Hkv, nsplit): a workgroup owns one (batch, kv head) and one
//    contiguous chunk of keys, and serves ALL M = (Hq/Hkv)*Sq query rows of
//    that kv head from a single read of K and V (GQA without expanded copies)
//  - D/8 lanes cover one key with one 16-byte load each, straight to VGPRs;
//    a wave covers 64/(D/8) keys per step, a block 4x that
//  - up to 8 rows the next step's K/V loads are issued before the current
//    step's arithmetic (one-step-ahead register prefetch)
//  - q stays packed bf16 in registers; scores accumulate in fp32 through
//    v_dot2_f32_bf16 and are reduced over the D/8 lanes with DPP adds
//  - every lane group runs its own fp32 online softmax (P is never rounded
//    to bf16); groups, then waves, merge once at the end
//  - nsplit == 1 writes bf16 output directly; otherwise per-split fp32
//    (m, l, acc[D]) partials go to a workspace and a second, plain launch
//    (decode_attn_combine_kernel) merges them
//
// pos0 is a kernel argument or is read from an int64 device tensor (1 or B
// elements) at run time, so a captured hipGraph follows the position.  The
// grid and the chunk length depend on Smax only.  The position is clamped
// to [0, Smax-Sq] before any address is formed.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "decode_attn_common.h"

template <int D, int MT>
__global__ __launch_bounds__(DA_BLOCK) void decode_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kc,
    const ushort* __restrict__ vc, ushort* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml,
    const long* __restrict__ pos_ptr, int pos_stride, long pos_host,
    int Hkv, int G, int Sq, int Smax, int chunk, int nsplit,
    long q_sb, long q_sh, long q_ss, long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss, long o_sb, long o_sh, long o_ss,
    float scale_log2) {
#define DA_SRC_INIT()                                                  \
  const ushort* kbase = kc + (long)b * k_sb + (long)h * k_sh + ld * 8; \
  const ushort* vbase = vc + (long)b * v_sb + (long)h * v_sh + ld * 8
#define DA_KPTR(j) (&kbase[(long)(j) * k_ss])
#define DA_VPTR(j) (&vbase[(long)(j) * v_ss])
#include "decode_attn_body.inc"
#undef DA_SRC_INIT
#undef DA_KPTR
#undef DA_VPTR
}

// Second launch: merge the per-split partials of one (batch, kv head, row).
// Only splits that start below the valid length were written; the rest of
// the workspace is never read.
template <int D>
__global__ __launch_bounds__(D) void decode_attn_combine_kernel(
    const float* __restrict__ part_acc, const float* __restrict__ part_ml,
    ushort* __restrict__ out, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int MT, long o_sb, long o_sh, long o_ss) {
  da_combine<D>(part_acc, part_ml, out, pos_ptr, pos_stride, pos_host, Hkv, G,
                Sq, Smax, chunk, nsplit, MT, o_sb, o_sh, o_ss);
}

static void da_check_kv(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 4 && t.stride(3) == 1,
              "decode_attention: ", name,
              " must be 4-D bf16 CUDA with contiguous head dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr()) % 16 == 0,
              "decode_attention: ", name,
              " must allow 16-byte loads (strides % 8, 16-byte base)");
}

// out: (B, Hq, Sq, D) bf16 view (any strides, contiguous head dim), written
// in place and returned.  pos_t: optional int64 device tensor (1 or B
// elements) that overrides pos0.  split_kv: chunk length override (0 = auto).
torch::Tensor decode_attention(torch::Tensor q, torch::Tensor k_cache,
                               torch::Tensor v_cache, torch::Tensor out,
                               c10::optional<torch::Tensor> pos_t, long pos0,
                               double scale, long split_kv) {
  da_check_kv(q, "q");
  da_check_kv(k_cache, "k_cache");
  da_check_kv(v_cache, "v_cache");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 &&
              out.dim() == 4 && out.stride(3) == 1);
  const int B = q.size(0), Hq = q.size(1), Sq = q.size(2), D = q.size(3);
  const int Hkv = k_cache.size(1);
  const long Smax_l = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "decode_attention: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_cache.size(0) == B && k_cache.size(3) == D &&
              v_cache.size(0) == B && v_cache.size(1) == Hkv &&
              v_cache.size(2) == Smax_l && v_cache.size(3) == D,
              "decode_attention: cache shape mismatch");
  TORCH_CHECK(out.size(0) == B && out.size(1) == Hq && out.size(2) == Sq &&
              out.size(3) == D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "decode_attention: Hq % Hkv != 0");
  TORCH_CHECK(Sq >= 1 && Smax_l >= Sq && Smax_l < (1L << 30));
  const int Smax = (int)Smax_l;
  const int G = Hq / Hkv;
  const int M = G * Sq;
  TORCH_CHECK(M <= DA_MAX_M, "decode_attention: (Hq/Hkv)*Sq = ", M,
              " exceeds the kernel's ", DA_MAX_M, " query rows per kv head");
  const long* pos_ptr = nullptr;
  int pos_stride = 0;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->is_cuda() && pos_t->scalar_type() == torch::kLong &&
                    pos_t->is_contiguous() &&
                    (pos_t->numel() == 1 || pos_t->numel() == B),
                "decode_attention: pos0 tensor must be int64 CUDA with 1 or "
                "B elements");
    pos_ptr = (const long*)pos_t->data_ptr();
    pos_stride = pos_t->numel() == 1 ? 0 : 1;
  } else {
    TORCH_CHECK(pos0 >= 0 && pos0 + Sq <= Smax, "decode_attention: pos0=",
                pos0, " with Sq=", Sq, " outside the cache (Smax=", Smax, ")");
  }
  TORCH_CHECK(split_kv >= 0);

  // split choice from Smax only, so a captured grid stays valid
  const int BH = B * Hkv;
  const int chunk = da_choose_chunk(
      Smax, BH, split_kv,
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  const int nsplit = (Smax + chunk - 1) / chunk;
  TORCH_CHECK(nsplit <= 65535);

  int MT = 1;
  while (MT < M) MT <<= 1;

  torch::Tensor part_acc, part_ml;
  float* pa = nullptr;
  float* pm = nullptr;
  if (nsplit > 1) {
    auto fopt = q.options().dtype(torch::kFloat);
    part_acc = torch::empty({BH, nsplit, MT, D}, fopt);
    part_ml = torch::empty({BH, nsplit, MT, 2}, fopt);
    pa = part_acc.data_ptr<float>();
    pm = part_ml.data_ptr<float>();
  }

  const float scale_log2 = (float)(scale * 1.4426950408889634);
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid((unsigned)BH, (unsigned)nsplit), block(DA_BLOCK);
  const ushort* qp = (const ushort*)q.data_ptr();
  const ushort* kp = (const ushort*)k_cache.data_ptr();
  const ushort* vp = (const ushort*)v_cache.data_ptr();
  ushort* op = (ushort*)out.data_ptr();
#define DA_LAUNCH(D_, MT_)                                                   \
  hipLaunchKernelGGL((decode_attn_kernel<D_, MT_>), grid, block, 0, stream,  \
                     qp, kp, vp, op, pa, pm, pos_ptr, pos_stride, pos0, Hkv, \
                     G, Sq, Smax, chunk, nsplit, q.stride(0), q.stride(1),   \
                     q.stride(2), k_cache.stride(0), k_cache.stride(1),      \
                     k_cache.stride(2), v_cache.stride(0), v_cache.stride(1),\
                     v_cache.stride(2), out.stride(0), out.stride(1),        \
                     out.stride(2), scale_log2)
#define DA_DISPATCH(D_)            \
  switch (MT) {                    \
    case 1: DA_LAUNCH(D_, 1); break;   \
    case 2: DA_LAUNCH(D_, 2); break;   \
    case 4: DA_LAUNCH(D_, 4); break;   \
    case 8: DA_LAUNCH(D_, 8); break;   \
    default: DA_LAUNCH(D_, 16); break; \
  }
  if (D == 64) { DA_DISPATCH(64) } else { DA_DISPATCH(128) }
#undef DA_DISPATCH
#undef DA_LAUNCH
  HIP_CHECK_LAST();
  if (nsplit > 1) {
    const dim3 cgrid((unsigned)BH, (unsigned)M);
#define DA_COMBINE(D_)                                                      \
  hipLaunchKernelGGL((decode_attn_combine_kernel<D_>), cgrid, dim3(D_), 0,  \
                     stream, pa, pm, op, pos_ptr, pos_stride, pos0, Hkv, G, \
                     Sq, Smax, chunk, nsplit, MT, out.stride(0),            \
                     out.stride(1), out.stride(2))
    if (D == 64) DA_COMBINE(64); else DA_COMBINE(128);
#undef DA_COMBINE
    HIP_CHECK_LAST();
  }
  return out;
}
