// Split-KV decode attention over an fp8 (OCP e4m3) KV cache, hd 64/128.
//
// The contract is decode_attn.hip's: q (B, Hq, Sq, D) bf16 attends to cache
// positions [0, pos0+i] per row, a workgroup owns one (batch, kv head) and
// one chunk of keys and serves all M = (Hq/Hkv)*Sq rows, every lane group
// runs its own fp32 online softmax, and groups, waves and splits merge as
// there.  The cache is the one kv_fp8.hip writes: D bytes of e4m3 and one
// fp32 power-of-two scale per (batch, kv head, position), for K and for V.
//
// What differs, because a key is half the bytes and the arithmetic per key
// is not:
//  - a lane owns EPL = 8 elements of a key (one 8-byte load, D/8 lanes per
//    key), which keeps the bf16 kernel's acc[MT][8] register layout.  16
//    elements per lane (16-byte loads, half the DPP reduction depth) were
//    built and measured for up to 4 rows: slower wherever a workgroup's
//    chunk is 1024 keys or less, 8 % faster only at 4096
//    (docs/design/kernels.md), so they are not instantiated
//  - a load step puts 2 arithmetic batches of keys in flight, so the bytes
//    in flight per lane match the bf16 kernel's at half the bytes per key;
//    the next step's loads are issued before this step's arithmetic
//  - K is converted once per key, shared by all rows: fp8 -> f32
//    (v_cvt_pk_f32_fp8) -> packed bf16 (exact, e4m3 fits bf16), and the
//    q.k dot stays on v_dot2_f32_bf16 against q packed in registers
//  - V goes fp8 -> f32 directly
//  - the K scale is folded with scale*log2(e) into one factor per key,
//    applied to the group-reduced score; the V scale multiplies p where
//    there are fewer rows than elements per lane (the row sum keeps the
//    unscaled p), the converted V slice otherwise
//  - one fp32 scale per key per lane group rides with the K/V loads of its
//    step, clamped to the same key index
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "decode_attn_common.h"

// no packed-fp32 VALU forms in this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

typedef float daf_fv2 __attribute__((ext_vector_type(2)));
typedef __bf16 daf_bv2 __attribute__((ext_vector_type(2)));

// two e4m3 bytes (the low or high half of w) as packed bf16, exact
template <bool HI>
DEVINL da_sv2 daf_fp8x2_to_bf16x2(uint w) {
  const daf_fv2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  return __builtin_bit_cast(da_sv2, __builtin_convertvector(f, daf_bv2));
}

template <int D, int MT>
__global__ __launch_bounds__(DA_BLOCK) void decode_attn_fp8_kernel(
    const ushort* __restrict__ q, const uint8_t* __restrict__ kc,
    const float* __restrict__ ksc, const uint8_t* __restrict__ vc,
    const float* __restrict__ vsc, ushort* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml,
    const long* __restrict__ pos_ptr, int pos_stride, long pos_host,
    int Hkv, int G, int Sq, int Smax, int chunk, int nsplit,
    long q_sb, long q_sh, long q_ss, long o_sb, long o_sh, long o_ss,
    float scale_log2) {
  constexpr int EPL = 8;                // elements of a key per lane
  constexpr int LPK = D / EPL;          // lanes per key
  constexpr int KPW = WAVE / LPK;       // keys per wave step
  constexpr int KPB = KPW * DA_WAVES;   // keys per block step
  constexpr int NW = EPL / 4;           // dwords of K (and of V) per lane
  constexpr int NP = EPL / 2;           // bf16 pairs per lane
  // keys per arithmetic batch (one online-softmax update) and per load step
  constexpr int UA = ((MT <= 4) ? 32 : 16) / EPL;
  constexpr int UL = 2 * UA;
  // V scale on p (MT multiplies per key) or on the V slice (EPL per key)
  constexpr bool VS_ON_P = MT < EPL;
  using VecT = uint2;                   // EPL bytes

  __shared__ float sm_acc[DA_WAVES * MT * D];
  __shared__ float sm_ml[DA_WAVES * MT * 2];

  const int bh = blockIdx.x;
  const int b = bh / Hkv, h = bh % Hkv;
  const int split = blockIdx.y;
  const int M = G * Sq;
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int len = p0 + Sq;              // <= Smax
  const int c0 = split * chunk;
  if (c0 >= len) return;                // empty split: block-uniform exit
  const int c1 = min(c0 + chunk, len);

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int ld = lane % LPK;            // which EPL-element slice of the head
  const int grp = wave * KPW + lane / LPK;

  uint qv[MT][NP];                      // packed bf16, this lane's d-slice
  int rowlim[MT];                       // last visible key of row m
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int e = 0; e < NP; ++e) qv[m][e] = 0;
    rowlim[m] = -1;                     // padding row: sees nothing
    if (m < M) {
      const int gq = m / Sq, i = m % Sq;
      const ushort* qp = &q[(long)b * q_sb + (long)(h * G + gq) * q_sh +
                            (long)i * q_ss + ld * EPL];
#pragma unroll
      for (int c = 0; c < EPL / 8; ++c) {
        const uint4 t = *(const uint4*)&qp[c * 8];
        qv[m][4 * c] = t.x;
        qv[m][4 * c + 1] = t.y;
        qv[m][4 * c + 2] = t.z;
        qv[m][4 * c + 3] = t.w;
      }
      rowlim[m] = p0 + i;
    }
  }

  float mrun[MT], lrun[MT], acc[MT][EPL];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    mrun[m] = -INFINITY;
    lrun[m] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[m][e] = 0.f;
  }

  const long row0 = (long)bh * Smax;    // caches are dense (B, Hkv, Smax, D)
  const uint8_t* kbase = kc + row0 * D + ld * EPL;
  const uint8_t* vbase = vc + row0 * D + ld * EPL;
  const float* ksbase = ksc + row0;
  const float* vsbase = vsc + row0;

  // K/V and their scales for one step: UL keys per lane.  The key index is
  // clamped into [c0, c1-1], so a lane past the end (and the prefetch past
  // the last step) re-reads the chunk's last key; its score is masked below.
  auto load_kv = [&](int base, VecT (&kv)[UL], VecT (&vv)[UL],
                     float (&ks)[UL], float (&vs)[UL]) {
#pragma unroll
    for (int u = 0; u < UL; ++u) {
      const int jc = min(base + u * KPB + grp, c1 - 1);
      kv[u] = *(const VecT*)&kbase[(long)jc * D];
      vv[u] = *(const VecT*)&vbase[(long)jc * D];
      ks[u] = ksbase[jc];
      vs[u] = vsbase[jc];
    }
  };

  // software pipeline as in the bf16 kernel: up to 8 rows the next step's
  // loads are requested before this step's arithmetic
  constexpr bool PF = MT <= 8;
  VecT kv[UL], vv[UL];
  float ks[UL], vs[UL];
  if (PF) load_kv(c0, kv, vv, ks, vs);
  for (int base = c0; base < c1; base += KPB * UL) {
    VecT kn[PF ? UL : 1], vn[PF ? UL : 1];
    float ksn[PF ? UL : 1], vsn[PF ? UL : 1];
    if constexpr (PF) {
      load_kv(base + KPB * UL, kn, vn, ksn, vsn);
    } else {
      load_kv(base, kv, vv, ks, vs);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u0 = 0; u0 < UL; u0 += UA) {
      int jl[UA];
      float kf[UA];
      da_sv2 kb[UA][NP];
      float vf[UA][EPL];
#pragma unroll
      for (int a = 0; a < UA; ++a) {
        const int j = base + (u0 + a) * KPB + grp;
        jl[a] = (j < c1) ? j : 0x7fffffff;
        kf[a] = ks[u0 + a] * scale_log2;
        const uint* kw = (const uint*)&kv[u0 + a];
        const uint* vw = (const uint*)&vv[u0 + a];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          kb[a][2 * w] = daf_fp8x2_to_bf16x2<false>(kw[w]);
          kb[a][2 * w + 1] = daf_fp8x2_to_bf16x2<true>(kw[w]);
          const daf_fv2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw[w], false);
          const daf_fv2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw[w], true);
          vf[a][4 * w] = lo.x;
          vf[a][4 * w + 1] = lo.y;
          vf[a][4 * w + 2] = hi.x;
          vf[a][4 * w + 3] = hi.y;
        }
        if constexpr (!VS_ON_P) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) vf[a][e] *= vs[u0 + a];
        }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const da_sv2* qp = (const da_sv2*)&qv[m][0];
        float s[UA];
        float mn = mrun[m];
#pragma unroll
        for (int a = 0; a < UA; ++a) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < NP; ++e)
            d = __builtin_amdgcn_fdot2_f32_bf16(kb[a][e], qp[e], d, false);
          d = da_group_sum<LPK>(d);
          s[a] = (jl[a] <= rowlim[m]) ? d * kf[a] : -INFINITY;
          mn = fmaxf(mn, s[a]);
        }
        // nothing visible yet: keep exp2(-inf - -inf) out of the arithmetic
        const float ms = (mn == -INFINITY) ? 0.f : mn;
        const float alpha = __builtin_amdgcn_exp2f(mrun[m] - ms);
        float p[UA], ps = 0.f;
#pragma unroll
        for (int a = 0; a < UA; ++a) {
          p[a] = __builtin_amdgcn_exp2f(s[a] - ms);
          ps += p[a];
          if constexpr (VS_ON_P) p[a] *= vs[u0 + a];
        }
        mrun[m] = mn;
        lrun[m] = lrun[m] * alpha + ps;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          float t = acc[m][e] * alpha;
#pragma unroll
          for (int a = 0; a < UA; ++a) t = fmaf(p[a], vf[a][e], t);
          acc[m][e] = t;
        }
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int u = 0; u < UL; ++u) {
        kv[u] = kn[u];
        vv[u] = vn[u];
        ks[u] = ksn[u];
        vs[u] = vsn[u];
      }
    }
  }

  // merge the lane groups of a wave (each ran its own online softmax)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float mx = mrun[m];
#pragma unroll
    for (int off = LPK; off < WAVE; off <<= 1)
      mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
    const float ms = (mx == -INFINITY) ? 0.f : mx;
    const float f = __builtin_amdgcn_exp2f(mrun[m] - ms);
    float l = lrun[m] * f;
#pragma unroll
    for (int off = LPK; off < WAVE; off <<= 1) l += __shfl_xor(l, off, WAVE);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      float a = acc[m][e] * f;
#pragma unroll
      for (int off = LPK; off < WAVE; off <<= 1)
        a += __shfl_xor(a, off, WAVE);
      acc[m][e] = a;
    }
    if (lane < LPK) {
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        sm_acc[(wave * MT + m) * D + ld * EPL + e] = acc[m][e];
      if (lane == 0) {
        sm_ml[(wave * MT + m) * 2] = mx;
        sm_ml[(wave * MT + m) * 2 + 1] = l;
      }
    }
  }
  __syncthreads();

  // merge the waves; one (row, d) element per thread per trip
  for (int idx = threadIdx.x; idx < M * D; idx += DA_BLOCK) {
    const int m = idx / D, d = idx % D;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w)
      mx = fmaxf(mx, sm_ml[(w * MT + m) * 2]);
    const float ms = (mx == -INFINITY) ? 0.f : mx;
    float l = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w) {
      const float f = __builtin_amdgcn_exp2f(sm_ml[(w * MT + m) * 2] - ms);
      l += sm_ml[(w * MT + m) * 2 + 1] * f;
      a += sm_acc[(w * MT + m) * D + d] * f;
    }
    if (nsplit == 1) {
      const int gq = m / Sq, i = m % Sq;
      out[(long)b * o_sb + (long)(h * G + gq) * o_sh + (long)i * o_ss + d] =
          f2bf(a / l);
    } else {
      const long row = ((long)bh * nsplit + split) * MT + m;
      part_acc[row * D + d] = a;
      if (d == 0) {
        part_ml[row * 2] = mx;
        part_ml[row * 2 + 1] = l;
      }
    }
  }
}

template <int D>
__global__ __launch_bounds__(D) void decode_attn_fp8_combine_kernel(
    const float* __restrict__ part_acc, const float* __restrict__ part_ml,
    ushort* __restrict__ out, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int MT, long o_sb, long o_sh, long o_ss) {
  da_combine<D>(part_acc, part_ml, out, pos_ptr, pos_stride, pos_host, Hkv, G,
                Sq, Smax, chunk, nsplit, MT, o_sb, o_sh, o_ss);
}

#pragma clang attribute pop

static void daf_check_cache(const torch::Tensor& data,
                            const torch::Tensor& scale, const char* name) {
  TORCH_CHECK(data.is_cuda() && data.scalar_type() == torch::kByte &&
                  data.dim() == 4 && data.is_contiguous() &&
                  ((uintptr_t)data.data_ptr()) % 16 == 0,
              "decode_attention: ", name,
              ".data must be contiguous 4-D uint8 CUDA, 16-byte aligned");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat &&
                  scale.dim() == 3 && scale.is_contiguous() &&
                  scale.size(0) == data.size(0) &&
                  scale.size(1) == data.size(1) &&
                  scale.size(2) == data.size(2),
              "decode_attention: ", name,
              ".scale must be contiguous fp32 (B, Hkv, Smax)");
}

// Same arguments as decode_attention, with each cache as (data, scale).
torch::Tensor decode_attention_fp8(torch::Tensor q, torch::Tensor k_data,
                                   torch::Tensor k_scale,
                                   torch::Tensor v_data,
                                   torch::Tensor v_scale, torch::Tensor out,
                                   c10::optional<torch::Tensor> pos_t,
                                   long pos0, double scale, long split_kv) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16 &&
                  q.dim() == 4 && q.stride(3) == 1,
              "decode_attention: q must be 4-D bf16 CUDA with contiguous "
              "head dim");
  TORCH_CHECK(q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0 &&
                  q.stride(2) % 8 == 0 &&
                  ((uintptr_t)q.data_ptr()) % 16 == 0,
              "decode_attention: q must allow 16-byte loads (strides % 8, "
              "16-byte base)");
  daf_check_cache(k_data, k_scale, "k_cache");
  daf_check_cache(v_data, v_scale, "v_cache");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 &&
              out.dim() == 4 && out.stride(3) == 1);
  const int B = q.size(0), Hq = q.size(1), Sq = q.size(2), D = q.size(3);
  const int Hkv = k_data.size(1);
  const long Smax_l = k_data.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "decode_attention: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_data.size(0) == B && k_data.size(3) == D &&
                  v_data.sizes() == k_data.sizes(),
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
  ushort* op = (ushort*)out.data_ptr();
#define DAF_LAUNCH(D_, MT_)                                                  \
  hipLaunchKernelGGL((decode_attn_fp8_kernel<D_, MT_>), grid, block,         \
                     0, stream, qp, k_data.data_ptr<uint8_t>(),              \
                     k_scale.data_ptr<float>(), v_data.data_ptr<uint8_t>(),  \
                     v_scale.data_ptr<float>(), op, pa, pm, pos_ptr,         \
                     pos_stride, pos0, Hkv, G, Sq, Smax, chunk, nsplit,      \
                     q.stride(0), q.stride(1), q.stride(2), out.stride(0),   \
                     out.stride(1), out.stride(2), scale_log2)
#define DAF_DISPATCH(D_)                \
  switch (MT) {                         \
    case 1: DAF_LAUNCH(D_, 1); break;   \
    case 2: DAF_LAUNCH(D_, 2); break;   \
    case 4: DAF_LAUNCH(D_, 4); break;   \
    case 8: DAF_LAUNCH(D_, 8); break;   \
    default: DAF_LAUNCH(D_, 16); break; \
  }
  if (D == 64) { DAF_DISPATCH(64) } else { DAF_DISPATCH(128) }
#undef DAF_DISPATCH
#undef DAF_LAUNCH
  HIP_CHECK_LAST();
  if (nsplit > 1) {
    const dim3 cgrid((unsigned)BH, (unsigned)M);
#define DAF_COMBINE(D_)                                                      \
  hipLaunchKernelGGL((decode_attn_fp8_combine_kernel<D_>), cgrid, dim3(D_),  \
                     0, stream, pa, pm, op, pos_ptr, pos_stride, pos0, Hkv,  \
                     G, Sq, Smax, chunk, nsplit, MT, out.stride(0),          \
                     out.stride(1), out.stride(2))
    if (D == 64) DAF_COMBINE(64); else DAF_COMBINE(128);
#undef DAF_COMBINE
    HIP_CHECK_LAST();
  }
  return out;
}
