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

#include "common.h"

#define DA_BLOCK 256
#define DA_WAVES (DA_BLOCK / WAVE)
#define DA_MAX_M 16

typedef short da_sv2 __attribute__((ext_vector_type(2)));

template <int CTRL>
DEVINL float da_dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF,
                                            0xF, false);
  return v + __int_as_float(t);
}

// all-reduce sum over aligned groups of LPK (8 or 16) lanes, VALU only
template <int LPK>
DEVINL float da_group_sum(float v) {
  if (LPK == 16) v = da_dpp_add<0x140>(v);  // row_mirror: i <-> 15-i
  v = da_dpp_add<0x141>(v);                 // row_half_mirror: i <-> 7-i
  v = da_dpp_add<0xB1>(v);                  // quad_perm [1,0,3,2]
  v = da_dpp_add<0x4E>(v);                  // quad_perm [2,3,0,1]
  return v;
}

DEVINL int da_read_pos(const long* pos_ptr, int pos_stride, long pos_host,
                       int b, int Smax, int Sq) {
  long p = pos_ptr ? pos_ptr[(long)b * pos_stride] : pos_host;
  // clamp BEFORE any address is formed: a stale position tensor may give a
  // wrong answer, never an out-of-range read
  const long hi = (long)Smax - Sq;
  p = p < 0 ? 0 : (p > hi ? hi : p);
  return (int)p;
}

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
  constexpr int LPK = D / 8;          // lanes per key (16 B each)
  constexpr int KPW = WAVE / LPK;     // keys per wave step
  constexpr int KPB = KPW * DA_WAVES; // keys per block step
  constexpr int U = (MT <= 4) ? 4 : 2;  // keys in flight per lane

  __shared__ float sm_acc[DA_WAVES * MT * D];
  __shared__ float sm_ml[DA_WAVES * MT * 2];

  const int bh = blockIdx.x;
  const int b = bh / Hkv, h = bh % Hkv;
  const int split = blockIdx.y;
  const int M = G * Sq;
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int len = p0 + Sq;            // <= Smax
  const int c0 = split * chunk;
  if (c0 >= len) return;              // empty split: block-uniform exit
  const int c1 = min(c0 + chunk, len);

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int ld = lane % LPK;          // which 8-element slice of the head dim
  const int grp = wave * KPW + lane / LPK;

  uint4 qv[MT];                       // packed bf16, this lane's d-slice
  int rowlim[MT];                     // last visible key of row m
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    qv[m] = make_uint4(0, 0, 0, 0);
    rowlim[m] = -1;                   // padding row: sees nothing
    if (m < M) {
      const int gq = m / Sq, i = m % Sq;
      qv[m] = *(const uint4*)&q[(long)b * q_sb + (long)(h * G + gq) * q_sh +
                                (long)i * q_ss + ld * 8];
      rowlim[m] = p0 + i;
    }
  }

  float mrun[MT], lrun[MT], acc[MT][8];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    mrun[m] = -INFINITY;
    lrun[m] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[m][e] = 0.f;
  }

  const ushort* kbase = kc + (long)b * k_sb + (long)h * k_sh + ld * 8;
  const ushort* vbase = vc + (long)b * v_sb + (long)h * v_sh + ld * 8;

  // K/V for one step: U keys per lane, 16 B each.  Addresses are clamped
  // into [c0, c1-1], so a lane past the end (and the prefetch past the last
  // step) re-reads the chunk's last key; its score is masked below.
  auto load_kv = [&](int base, uint4 (&kv)[U], uint4 (&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jc = min(base + u * KPB + grp, c1 - 1);
      kv[u] = *(const uint4*)&kbase[(long)jc * k_ss];
      vv[u] = *(const uint4*)&vbase[(long)jc * v_ss];
    }
  };

  // software pipeline: the next step's K/V are requested before this step's
  // arithmetic (up to 16 rows there are registers for it), and the
  // scheduler may not sink the loads down to their first use
  constexpr bool PF = MT <= 8;
  uint4 kv[U], vv[U];
  if (PF) load_kv(c0, kv, vv);
  for (int base = c0; base < c1; base += KPB * U) {
    uint4 kn[PF ? U : 1], vn[PF ? U : 1];
    if constexpr (PF) {
      load_kv(base + KPB * U, kn, vn);
    } else {
      load_kv(base, kv, vv);
    }
    __builtin_amdgcn_sched_barrier(0);
    int jl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = base + u * KPB + grp;
      jl[u] = (j < c1) ? j : 0x7fffffff;
    }
    float vf[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint* w = (const uint*)&vv[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vf[u][2 * e] = __uint_as_float(w[e] << 16);
        vf[u][2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const da_sv2* qp = (const da_sv2*)&qv[m];
      float s[U];
      float mn = mrun[m];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const da_sv2* kp = (const da_sv2*)&kv[u];
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a = __builtin_amdgcn_fdot2_f32_bf16(kp[e], qp[e], a, false);
        a = da_group_sum<LPK>(a);
        s[u] = (jl[u] <= rowlim[m]) ? a * scale_log2 : -INFINITY;
        mn = fmaxf(mn, s[u]);
      }
      // nothing visible yet: keep exp2(-inf - -inf) out of the arithmetic
      const float ms = (mn == -INFINITY) ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(mrun[m] - ms);
      float p[U], ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        p[u] = __builtin_amdgcn_exp2f(s[u] - ms);
        ps += p[u];
      }
      mrun[m] = mn;
      lrun[m] = lrun[m] * alpha + ps;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = acc[m][e] * alpha;
#pragma unroll
        for (int u = 0; u < U; ++u) t = fmaf(p[u], vf[u][e], t);
        acc[m][e] = t;
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        kv[u] = kn[u];
        vv[u] = vn[u];
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
    for (int e = 0; e < 8; ++e) {
      float a = acc[m][e] * f;
#pragma unroll
      for (int off = LPK; off < WAVE; off <<= 1)
        a += __shfl_xor(a, off, WAVE);
      acc[m][e] = a;
    }
    if (lane < LPK) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        sm_acc[(wave * MT + m) * D + ld * 8 + e] = acc[m][e];
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

// Second launch: merge the per-split partials of one (batch, kv head, row).
// Only splits that start below the valid length were written; the rest of
// the workspace is never read.
template <int D>
__global__ __launch_bounds__(D) void decode_attn_combine_kernel(
    const float* __restrict__ part_acc, const float* __restrict__ part_ml,
    ushort* __restrict__ out, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int MT, long o_sb, long o_sh, long o_ss) {
  const int bh = blockIdx.x, m = blockIdx.y, d = threadIdx.x;
  const int b = bh / Hkv, h = bh % Hkv;
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int len = p0 + Sq;
  const int nvalid = min(nsplit, (len + chunk - 1) / chunk);
  const long row0 = (long)bh * nsplit * MT + m;
  // the loads of different splits are independent: unroll so that several
  // are in flight (a serial chain of nsplit misses dominated at batch 1)
  float mx = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < nvalid; ++s)
    mx = fmaxf(mx, part_ml[(row0 + (long)s * MT) * 2]);
  // split 0 always holds key 0, which every row sees, so mx is finite
  float l = 0.f, a = 0.f;
#pragma unroll 8
  for (int s = 0; s < nvalid; ++s) {
    const long row = row0 + (long)s * MT;
    const float f = __builtin_amdgcn_exp2f(part_ml[row * 2] - mx);
    l += part_ml[row * 2 + 1] * f;
    a += part_acc[row * D + d] * f;
  }
  const int gq = m / Sq, i = m % Sq;
  out[(long)b * o_sb + (long)(h * G + gq) * o_sh + (long)i * o_ss + d] =
      f2bf(a / l);
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
  int chunk;
  if (split_kv > 0) {
    chunk = (int)std::min<long>((split_kv + 63) / 64 * 64, 1L << 30);
  } else {
    const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const int want = std::max(1, (2 * cus + BH - 1) / BH);
    chunk = ((Smax + want - 1) / want + 63) / 64 * 64;
  }
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
