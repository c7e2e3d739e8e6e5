// Split-KV chunk attention over a KV cache, bf16, head dim 64/128 (gfx950):
// the kernel for 17..64 query rows per kv head (speculative verification,
// small chunked-prefill steps), between decode_attn.hip (v_dot2, <= 16 rows)
// and prefill_attn.hip (MFMA, no split-KV).
//
// q (B, Hq, Sq, D) holds Sq new positions per batch element; they attend to
// the un-expanded caches (B, Hkv, Smax, D).  Row m of a kv head is query head
// m / Sq at position i = m % Sq and sees cache positions [0, pos_b + i]; the
// contract of decode_attn.hip with M = (Hq/Hkv)*Sq up to 64.
//
// Work split
//  - grid (nsplit, B*Hkv), 256 threads.  A workgroup owns one (batch, kv
//    head), one contiguous chunk of keys and ALL M rows as RT = 1, 2 or 4
//    16-row MFMA tiles: every query head of the kv head is served from one
//    read of K and V.
//  - the four waves split the chunk's KEYS: wave w takes the 32-key steps
//    w, w+4, ...  Each wave keeps its own fp32 online-softmax state and its
//    own output accumulators for all RT tiles, so there is NO workgroup
//    barrier in the key loop; the waves merge once through LDS at the end.
//
// Everything is computed transposed, which keeps P in registers:
//    S^T = K Q^T     A = K fragment, B = q fragment
//    O^T += V^T P^T  A = V^T fragment, B = P fragment
// The C layout of v_mfma_f32_16x16x32_bf16 (col = lane & 15, row =
// (lane >> 4) * 4 + reg) puts query row l15 = lane & 15 in every lane of both
// products, so a lane's softmax state (m, l) and its rescale factor belong to
// ONE query row, and the 8 scores a lane holds of a 32-key step (keys
// lg*4..+3 and 16 + lg*4..+3, lg = lane >> 4) are, rounded to bf16, exactly
// the B fragment of the second product once V^T is stored with its keys in
// the same order.  P never goes through LDS.
//
// Data movement
//  - K: global memory straight into A fragments.  A lane's 8 bf16 are 16
//    contiguous bytes of one key row: one 16-byte load, no LDS.  A fragment
//    is loaded once per step and used by all RT row tiles.
//  - V: a lane loads the same 8-wide d slice of D/16 keys (16 bytes each),
//    transposes the 8 x D/16 block in registers (one v_perm per dword) and
//    writes it as 8 rows of V^T[d][key] into the wave's private LDS slab
//    (XOR-swizzled, keys in fragment order); fragments come back with one
//    ds_read_b128 each and serve all RT tiles.  The slab is wave-private:
//    LDS operations of one wave complete in order, no barrier is needed.
//  - the next step's K and V loads are issued before the current step's
//    MFMAs (sched_barrier keeps them there).
//  - q: staged once per workgroup in LDS (swizzled), one barrier at entry;
//    RT <= 2 keeps its fragments in registers, RT = 4 re-reads them per step.
//
// Causality: keys at or past pos_b + Sq are never loaded (zeros are staged),
// scores are masked by select and only in key tiles that cross a row tile's
// diagonal, and a row tile skips the MFMAs of a key tile it sees nothing of.
// pos is a host argument or read on the device (da_read_pos, clamped before
// any address is formed); nsplit and the chunk come from da_choose_chunk
// (Smax and the CU count only), so a captured launch follows the position.
//
// Output: nsplit == 1 writes bf16 directly; otherwise fp32 (m, l, acc[D])
// partials in the workspace layout of decode_attn.hip, merged by da_combine.
// No atomics, no scratch.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

// no packed-fp32 VALU forms in this file's kernels; the shared headers are
// included under the attribute so that their inlines still inline
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

#include "decode_attn_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 ca_bf16x8;
typedef __attribute__((ext_vector_type(4))) float ca_f32x4;
// vector types of this file's own: the HIP headers' make_uint4 and friends
// are functions without the attribute above and would not inline
typedef __attribute__((ext_vector_type(4))) unsigned int ca_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int ca_u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned short ca_u16x4;

constexpr int CA_KT = 32;      // keys per wave step
constexpr int CA_NW = 4;       // waves per workgroup
constexpr int CA_MAX_M = 64;   // query rows per kv head

DEVINL int ca_min(int a, int b) { return a < b ? a : b; }

// workgroup barrier with LDS visibility, from builtins only
DEVINL void ca_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// value of lane (lane ^ X), X = 16 or 32
template <int X>
DEVINL float ca_xor(float v, int lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ X) << 2,
                                          __builtin_bit_cast(int, v)));
}

// swizzled index (in shorts) into the q tile, [rows][D] with 2*D-byte rows
template <int D>
DEVINL int ca_swzD(int row, int col) {
  return row * D + (col ^ ((row & (D / 8 - 1)) << 3));
}

// swizzled index (in shorts) into a V^T slab, [D][32] with 64-byte rows
DEVINL int ca_swz32(int row, int col) {
  return row * CA_KT + (col ^ (((row >> 2) & 3) << 3));
}

// swizzled index (in floats) into a merge slab, [16][D]; c4 = d / 4
template <int D>
DEVINL int ca_swzF(int row, int c4) { return row * D + ((c4 ^ row) << 2); }

template <int D, int RT>
__launch_bounds__(CA_NW * 64)
__global__ void chunk_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kc,
    const ushort* __restrict__ vc, ushort* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml,
    const long* __restrict__ pos_ptr, int pos_stride, long pos_host, int Hkv,
    int G, int Sq, int Smax, int chunk, int nsplit, long q_sb, long q_sh,
    long q_ss, long k_sb, long k_sh, long k_ss, long v_sb, long v_sh,
    long v_ss, long o_sb, long o_sh, long o_ss, float scale_log2) {
  constexpr int KC = D / 32;        // 32-wide chunks of the head dim (S^T)
  constexpr int DC = D / 16;        // 16-wide groups of the head dim (O^T)
  constexpr int LPR = D / 8;        // lanes per V row (16 B each)
  constexpr int KPL = D / 16;       // keys a lane loads of a 32-key V tile
  constexpr int MT = RT * 16;       // rows in the workspace layout
  constexpr bool QREG = RT <= 2;    // q fragments live in registers
  constexpr int SLAB = 16 * D;      // floats per wave slab (= 32*D shorts)

  // one array carved by hand: the q tile, the four wave slabs (V^T in the
  // key loop, the fp32 merge tile after it) and the waves' (m, l)
  __shared__ __attribute__((aligned(16))) float smem[MT * D / 2 + CA_NW * SLAB + CA_NW * MT * 2];
  ushort* q_lds = (ushort*)smem;
  float* slabs = smem + MT * D / 2;
  float* sm_ml = slabs + CA_NW * SLAB;

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int split = __builtin_amdgcn_workgroup_id_x();
  const int bh = __builtin_amdgcn_workgroup_id_y();
  const int b = bh / Hkv, h = bh % Hkv;
  const int M = G * Sq;
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int len = p0 + Sq;          // <= Smax
  const int c0 = split * chunk;
  if (c0 >= len) return;            // empty split: block-uniform exit
  const int c1 = ca_min(c0 + chunk, len);

  // stage q: row m is head m / Sq, position m % Sq; padding rows are zero
  for (int idx = tid; idx < MT * LPR; idx += CA_NW * 64) {
    const int m = idx / LPR, col = (idx % LPR) * 8;
    ca_u32x4 v = (ca_u32x4)(0u);
    if (m < M) {
      const int gq = m / Sq, i = m % Sq;
      v = *(const ca_u32x4*)&q[(long)b * q_sb + (long)(h * G + gq) * q_sh +
                            (long)i * q_ss + col];
    }
    *(ca_u32x4*)&q_lds[ca_swzD<D>(m, col)] = v;
  }
  ca_barrier();

  // per row tile: the lane's row limit and the tile's wave-uniform extremes.
  // Padding rows take the last row's limit; they are never written out.
  int lim[RT], tmin[RT], tmax[RT];
  bool act[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int mlo = t * 16, mhi = ca_min(t * 16 + 15, M - 1);
    act[t] = mlo < M;
    lim[t] = p0 + ca_min(mlo + l15, M - 1) % Sq;
    const bool one_head = act[t] && mlo / Sq == mhi / Sq;
    tmin[t] = p0 + (one_head ? mlo % Sq : 0);
    tmax[t] = p0 + (one_head ? mhi % Sq : Sq - 1);
  }

  auto q_frag = [&](int t, int c) {
    return *(const ca_bf16x8*)&q_lds[ca_swzD<D>(t * 16 + l15, c * 32 + lg * 8)];
  };
  ca_bf16x8 b_q[QREG ? RT : 1][KC];
  if constexpr (QREG) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int c = 0; c < KC; ++c) b_q[t][c] = q_frag(t, c);
  }

  float m_run[RT], l_run[RT];       // of query row t*16 + l15
  ca_f32x4 acc_o[RT][DC];           // O^T: d = dg*16 + lg*4 + reg, row l15
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
#pragma unroll
    for (int dg = 0; dg < DC; ++dg) acc_o[t][dg] = (ca_f32x4)(0.f);
  }

  const ushort* kp = kc + (long)b * k_sb + (long)h * k_sh + lg * 8;
  const ushort* vp = vc + (long)b * v_sb + (long)h * v_sh;

  // V staging: this lane's d slice and keys.  Local key of load u and the
  // column it lands in keep the fragment order: key kg*16 + g*4 + r sits in
  // column g*8 + kg*4 + r, so columns g*8..+7 are lane group g's 8 keys.
  const int vds = lane % LPR, vkg = lane / LPR;
  const int vgrp = D == 128 ? vkg : (vkg & 3);
  const int vcol = D == 128 ? vkg * 8 : (vkg & 3) * 8 + (vkg >> 2) * 4;
  vp += vds * 8;
  ushort* slab = (ushort*)(slabs + wid * SLAB);

  // keys at or past c1 are never loaded: dead slots may hold anything
  auto load_k = [&](int kt0, ca_bf16x8 (&kf)[2][KC]) {
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      const int key = kt0 + kg * 16 + l15;
#pragma unroll
      for (int c = 0; c < KC; ++c)
        kf[kg][c] = key < c1
                        ? *(const ca_bf16x8*)&kp[(long)key * k_ss + c * 32]
                        : (ca_bf16x8)(__bf16)0.f;
    }
  };
  auto load_v = [&](int kt0, ca_u32x4 (&vr)[KPL]) {
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
      const int kloc = D == 128 ? (u >> 2) * 16 + vgrp * 4 + (u & 3)
                                : (vkg >> 2) * 16 + vgrp * 4 + u;
      const int key = kt0 + kloc;
      vr[u] = key < c1 ? *(const ca_u32x4*)&vp[(long)key * v_ss]
                       : (ca_u32x4)(0u);
    }
  };
  // 8 x KPL block of (d, key) transposed in registers, one row of V^T per
  // store (16 bytes at D = 128, 8 at D = 64)
  auto stage_v = [&](const ca_u32x4 (&vr)[KPL]) {
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      uint lo[KPL / 2], hi[KPL / 2];
#pragma unroll
      for (int j = 0; j < KPL / 2; ++j) {
        const uint a = ((const uint*)&vr[2 * j])[e2];
        const uint c = ((const uint*)&vr[2 * j + 1])[e2];
        lo[j] = (a & 0xffffu) | (c << 16);
        hi[j] = (a >> 16) | (c & 0xffff0000u);
      }
      const int d = vds * 8 + e2 * 2;
      if constexpr (D == 128) {
        *(ca_u32x4*)&slab[ca_swz32(d, vcol)] = (ca_u32x4){lo[0], lo[1], lo[2], lo[3]};
        *(ca_u32x4*)&slab[ca_swz32(d + 1, vcol)] = (ca_u32x4){hi[0], hi[1], hi[2], hi[3]};
      } else {
        *(ca_u32x2*)&slab[ca_swz32(d, vcol)] = (ca_u32x2){lo[0], lo[1]};
        *(ca_u32x2*)&slab[ca_swz32(d + 1, vcol)] = (ca_u32x2){hi[0], hi[1]};
      }
    }
  };

  constexpr int STRIDE = CA_NW * CA_KT;
  int kt0 = c0 + wid * CA_KT;
  ca_bf16x8 k_cur[2][KC];
  ca_u32x4 v_reg[KPL];
  if (kt0 < c1) {
    load_k(kt0, k_cur);
    load_v(kt0, v_reg);
  }
  for (; kt0 < c1; kt0 += STRIDE) {
    stage_v(v_reg);
    ca_bf16x8 k_nxt[2][KC];
    // past the chunk both loaders stage zeros without touching memory
    load_k(kt0 + STRIDE, k_nxt);
    load_v(kt0 + STRIDE, v_reg);
    __builtin_amdgcn_sched_barrier(0);

    ca_bf16x8 a_v[DC];
#pragma unroll
    for (int dg = 0; dg < DC; ++dg)
      a_v[dg] = *(const ca_bf16x8*)&slab[ca_swz32(dg * 16 + l15, lg * 8)];

#pragma unroll
    for (int t = 0; t < RT; ++t) {
      // wave-uniform: the tile's rows see nothing of this key tile
      if (!act[t] || kt0 > tmax[t]) continue;

      ca_f32x4 s[2];
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        s[kg] = (ca_f32x4)(0.f);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          ca_bf16x8 bq;
          if constexpr (QREG) bq = b_q[t][c]; else bq = q_frag(t, c);
          s[kg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_cur[kg][c], bq,
                                                          s[kg], 0, 0, 0);
        }
      }
#pragma unroll
      for (int kg = 0; kg < 2; ++kg)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kg][r] *= scale_log2;
      // the key tile crosses the diagonal if its last key is hidden from
      // the row tile's first row; only then is the mask evaluated
      if (kt0 + CA_KT - 1 > tmin[t]) {
#pragma unroll
        for (int kg = 0; kg < 2; ++kg)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kt0 + kg * 16 + lg * 4 + r;
            s[kg][r] = key <= lim[t] ? s[kg][r] : -INFINITY;
          }
      }

      float tm = s[0][0];
#pragma unroll
      for (int r = 1; r < 4; ++r) tm = __builtin_fmaxf(tm, s[0][r]);
#pragma unroll
      for (int r = 0; r < 4; ++r) tm = __builtin_fmaxf(tm, s[1][r]);
      tm = __builtin_fmaxf(tm, ca_xor<16>(tm, lane));
      tm = __builtin_fmaxf(tm, ca_xor<32>(tm, lane));
      const float mn = __builtin_fmaxf(m_run[t], tm);
      // nothing visible yet: keep exp2(-inf - -inf) out of the arithmetic
      const float ms = (mn == -INFINITY) ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(m_run[t] - ms);
      m_run[t] = mn;
      ca_bf16x8 b_p;
      float psum = 0.f;           // this lane's 8 keys; lanes add at the end
#pragma unroll
      for (int kg = 0; kg < 2; ++kg)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(s[kg][r] - ms);
          psum += p;
          b_p[kg * 4 + r] = (__bf16)p;
        }
      l_run[t] = l_run[t] * alpha + psum;
#pragma unroll
      for (int dg = 0; dg < DC; ++dg) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[t][dg][r] *= alpha;
        acc_o[t][dg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_v[dg], b_p, acc_o[t][dg], 0, 0, 0);
      }
    }
#pragma unroll
    for (int kg = 0; kg < 2; ++kg)
#pragma unroll
      for (int c = 0; c < KC; ++c) k_cur[kg][c] = k_nxt[kg][c];
  }

  // ---- merge the four waves, one row tile at a time through the slabs ----
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    float l = l_run[t];
    l += ca_xor<16>(l, lane);
    l += ca_xor<32>(l, lane);
    if (lg == 0) {
      sm_ml[(wid * MT + t * 16 + l15) * 2] = m_run[t];
      sm_ml[(wid * MT + t * 16 + l15) * 2 + 1] = l;
    }
  }
  float* myslab = slabs + wid * SLAB;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (!act[t]) continue;          // block-uniform
    if (t > 0) ca_barrier();        // the previous tile has been read
#pragma unroll
    for (int dg = 0; dg < DC; ++dg)
      *(ca_f32x4*)&myslab[ca_swzF<D>(l15, dg * 4 + lg)] = acc_o[t][dg];
    ca_barrier();
    for (int idx = tid; idx < 16 * (D / 4); idx += CA_NW * 64) {
      const int row = idx / (D / 4), c4 = idx % (D / 4);
      const int m = t * 16 + row;
      if (m >= M) continue;
      float mw[CA_NW], mx = -INFINITY;
#pragma unroll
      for (int w = 0; w < CA_NW; ++w) {
        mw[w] = sm_ml[(w * MT + m) * 2];
        mx = __builtin_fmaxf(mx, mw[w]);
      }
      const float ms = (mx == -INFINITY) ? 0.f : mx;
      float l = 0.f;
      ca_f32x4 a = (ca_f32x4)(0.f);
#pragma unroll
      for (int w = 0; w < CA_NW; ++w) {
        const float f = __builtin_amdgcn_exp2f(mw[w] - ms);
        l += sm_ml[(w * MT + m) * 2 + 1] * f;
        const ca_f32x4 aw = *(const ca_f32x4*)&slabs[w * SLAB + ca_swzF<D>(row, c4)];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] += aw[r] * f;
      }
      if (nsplit == 1) {
        // key 0 is in the only split and every row sees it: l > 0
        const int gq = m / Sq, i = m % Sq;
        ca_u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(a[r] / l);
        *(ca_u16x4*)&out[(long)b * o_sb + (long)(h * G + gq) * o_sh +
                        (long)i * o_ss + c4 * 4] = o;
      } else {
        // a row that sees nothing of this split: m = -inf, l = 0, acc = 0
        const long prow = ((long)bh * nsplit + split) * MT + m;
        *(ca_f32x4*)&part_acc[prow * D + c4 * 4] = a;
        if (c4 == 0) {
          part_ml[prow * 2] = mx;
          part_ml[prow * 2 + 1] = l;
        }
      }
    }
  }
}

// Second launch: da_combine as it is (grid (B*Hkv, M), D threads)
template <int D>
__global__ __launch_bounds__(D) void chunk_attn_combine_kernel(
    const float* __restrict__ part_acc, const float* __restrict__ part_ml,
    ushort* __restrict__ out, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int MT, long o_sb, long o_sh, long o_ss) {
  da_combine<D>(part_acc, part_ml, out, pos_ptr, pos_stride, pos_host, Hkv, G,
                Sq, Smax, chunk, nsplit, MT, o_sb, o_sh, o_ss);
}

}  // namespace

#pragma clang attribute pop

static void ca_check_kv(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 4 && t.stride(3) == 1,
              "chunk_attention: ", name,
              " must be 4-D bf16 CUDA with contiguous head dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr()) % 16 == 0,
              "chunk_attention: ", name,
              " must allow 16-byte loads (strides % 8, 16-byte base)");
}

// out: (B, Hq, Sq, D) bf16 view (any strides a multiple of 4, contiguous head
// dim), written in place and returned.  pos_t: optional int64 device tensor
// (1 or B elements) that overrides pos0.  split_kv: chunk length override
// (0 = auto).
torch::Tensor chunk_attention(torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor out,
                              c10::optional<torch::Tensor> pos_t, long pos0,
                              double scale, long split_kv) {
  ca_check_kv(q, "q");
  ca_check_kv(k_cache, "k_cache");
  ca_check_kv(v_cache, "v_cache");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 &&
              out.dim() == 4 && out.stride(3) == 1);
  TORCH_CHECK(out.stride(0) % 4 == 0 && out.stride(1) % 4 == 0 &&
                  out.stride(2) % 4 == 0 &&
                  ((uintptr_t)out.data_ptr()) % 8 == 0,
              "chunk_attention: out must allow 8-byte stores");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  const long Sq_l = q.size(2);
  const int Hkv = k_cache.size(1);
  const long Smax_l = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "chunk_attention: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_cache.size(0) == B && k_cache.size(3) == D &&
              v_cache.size(0) == B && v_cache.size(1) == Hkv &&
              v_cache.size(2) == Smax_l && v_cache.size(3) == D,
              "chunk_attention: cache shape mismatch");
  TORCH_CHECK(out.size(0) == B && out.size(1) == Hq && out.size(2) == Sq_l &&
              out.size(3) == D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "chunk_attention: Hq % Hkv != 0");
  TORCH_CHECK(B >= 1 && Sq_l >= 1 && Smax_l >= Sq_l && Smax_l < (1L << 30),
              "chunk_attention: need 1 <= Sq <= Smax < 2^30, got Sq=", Sq_l,
              " Smax=", Smax_l);
  const int Sq = (int)Sq_l, Smax = (int)Smax_l;
  const int G = Hq / Hkv;
  const long M_l = (long)G * Sq;
  TORCH_CHECK(M_l <= CA_MAX_M, "chunk_attention: (Hq/Hkv)*Sq = ", M_l,
              " exceeds the kernel's ", CA_MAX_M, " query rows per kv head");
  const int M = (int)M_l;
  const long* pos_ptr = nullptr;
  int pos_stride = 0;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->is_cuda() && pos_t->scalar_type() == torch::kLong &&
                    pos_t->is_contiguous() &&
                    (pos_t->numel() == 1 || pos_t->numel() == B),
                "chunk_attention: pos0 tensor must be int64 CUDA with 1 or "
                "B elements");
    pos_ptr = (const long*)pos_t->data_ptr();
    pos_stride = pos_t->numel() == 1 ? 0 : 1;
  } else {
    TORCH_CHECK(pos0 >= 0 && pos0 + Sq <= Smax, "chunk_attention: pos0=",
                pos0, " with Sq=", Sq, " outside the cache (Smax=", Smax, ")");
  }
  TORCH_CHECK(split_kv >= 0);

  // split choice from Smax only, so a captured grid stays valid
  const long BH = (long)B * Hkv;
  TORCH_CHECK(BH <= 65535, "chunk_attention: B*Hkv = ", BH,
              " exceeds the grid's y extent");
  const int chunk = da_choose_chunk(
      Smax, (int)BH, split_kv,
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  const int nsplit = (Smax + chunk - 1) / chunk;
  const int RT = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  const int MT = RT * 16;

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
  const dim3 grid((unsigned)nsplit, (unsigned)BH), block(CA_NW * 64);
  const ushort* qp = (const ushort*)q.data_ptr();
  const ushort* kp = (const ushort*)k_cache.data_ptr();
  const ushort* vp = (const ushort*)v_cache.data_ptr();
  ushort* op = (ushort*)out.data_ptr();
#define CA_LAUNCH(D_, RT_)                                                    \
  hipLaunchKernelGGL((chunk_attn_kernel<D_, RT_>), grid, block, 0, stream,    \
                     qp, kp, vp, op, pa, pm, pos_ptr, pos_stride, pos0, Hkv,  \
                     G, Sq, Smax, chunk, nsplit, q.stride(0), q.stride(1),    \
                     q.stride(2), k_cache.stride(0), k_cache.stride(1),       \
                     k_cache.stride(2), v_cache.stride(0), v_cache.stride(1), \
                     v_cache.stride(2), out.stride(0), out.stride(1),         \
                     out.stride(2), scale_log2)
#define CA_DISPATCH(D_)                \
  switch (RT) {                        \
    case 1: CA_LAUNCH(D_, 1); break;   \
    case 2: CA_LAUNCH(D_, 2); break;   \
    default: CA_LAUNCH(D_, 4); break;  \
  }
  if (D == 64) { CA_DISPATCH(64) } else { CA_DISPATCH(128) }
#undef CA_DISPATCH
#undef CA_LAUNCH
  HIP_CHECK_LAST();
  if (nsplit > 1) {
    const dim3 cgrid((unsigned)BH, (unsigned)M);
#define CA_COMBINE(D_)                                                      \
  hipLaunchKernelGGL((chunk_attn_combine_kernel<D_>), cgrid, dim3(D_), 0,   \
                     stream, pa, pm, op, pos_ptr, pos_stride, pos0, Hkv, G, \
                     Sq, Smax, chunk, nsplit, MT, out.stride(0),            \
                     out.stride(1), out.stride(2))
    if (D == 64) CA_COMBINE(64); else CA_COMBINE(128);
#undef CA_COMBINE
    HIP_CHECK_LAST();
  }
  return out;
}
