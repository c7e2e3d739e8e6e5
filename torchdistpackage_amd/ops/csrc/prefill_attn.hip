// Flash-prefill attention over a KV cache, bf16, head dim 64/128 (gfx950).
//
// q (B, Hq, Sq, D) holds Sq new query positions per batch element; they
// attend to the un-expanded caches (B, Hkv, Smax, D).  Row i of batch b sees
// cache positions [0, pos_b + i] (bottom-right aligned causal mask), the
// contract of decode_attn.hip without its 16-row cap: prompt prefill,
// chunked prefill and speculative verification are all this shape.
//
// Work split
//  - grid (position tiles, B*Hkv).  A workgroup (8 waves) owns one (batch,
//    kv head), a tile of 16*ptw consecutive query positions, and ALL
//    G = Hq/Hkv query heads of that kv head.
//  - a wave tile is 16 consecutive positions of one query head; the
//    workgroup's G*ptw <= 16 wave tiles go to the 8 waves round-robin (TPW =
//    1 or 2 tiles per wave, all state in registers).  ptw is chosen on the
//    host from G (16/G, so any G in 1..16 fills the waves) and lowered while
//    the grid would leave CUs idle.
//  - every 32-key K/V tile is staged in LDS once per workgroup and serves
//    every wave tile of all G heads: HBM reads of K/V per (kv head, position
//    tile) do not scale with G.
//  - position tiles are issued last-first: the tiles with the longest key
//    loops start before the short ones.
//
// Data movement: K[key][d] in XOR-swizzled LDS (swzD), V transposed to
// V^T[d][key] (swz32), both B operands of v_mfma_f32_16x16x32_bf16 read with
// one ds_read_b128 per fragment.  Each thread owns one 16-byte chunk of the
// K and of the V tile; the next tile's global loads are issued right after
// the LDS write barrier and fly under the current tile's MFMAs.
//
// Math: S = Q K^T and O += P V on v_mfma_f32_16x16x32_bf16 (A/B: 8 bf16 per
// lane, K-contiguous; C: col = lane&15, row = (lane>>4)*4 + reg).  fp32
// online softmax in the exp2 domain (scale*log2e folded into one multiply),
// P rounded to bf16 once for the PV MFMA, the output normalised in fp32 and
// rounded once.
//
// Causality: the key loop of a position tile ends at its own frontier,
// pos + tile_end, read on the device, so the grid never depends on pos and a
// captured launch follows a position tensor.  Keys at or past the frontier
// are never loaded (zeros are staged for K and V instead), so nothing past
// pos + Sq reaches the result and nothing past Smax is read.  Scores are
// masked by select, and only in tiles that cross a wave tile's diagonal; a
// wave whose rows see nothing of a key tile skips its MFMAs but still
// reaches the barriers.  No atomics, no scratch.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "common.h"

// no packed-fp32 VALU forms in this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 pa_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pa_f32x4;

constexpr int PA_WQ = 16;    // query positions per wave tile
constexpr int PA_KT = 32;    // keys per LDS tile
constexpr int PA_NW = 8;     // waves per workgroup
constexpr int PA_MAX_G = 16; // query heads per kv head
constexpr int PA_MAX_TILES = 2 * PA_NW;  // wave tiles per workgroup

DEVINL pa_bf16x8 pa_pack8(const unsigned short* p) {
  return *(const pa_bf16x8*)p;
}

// swizzled index (in shorts) into a [rows][D] tile with 2*D-byte rows
template <int D>
DEVINL int pa_swzD(int row, int col) {
  return row * D + (col ^ ((row & (D / 8 - 1)) << 3));
}

// swizzled index into a [rows][32] tile (64-byte rows)
DEVINL int pa_swz32(int row, int col) {
  return row * PA_KT + (col ^ (((row >> 2) & 3) << 3));
}

DEVINL int pa_read_pos(const long* pos_ptr, int pos_stride, long pos_host,
                       int b, int Smax, int Sq) {
  long p = pos_ptr ? pos_ptr[(long)b * pos_stride] : pos_host;
  // clamp BEFORE any address is formed: a stale position tensor may give a
  // wrong answer, never an out-of-range read
  const long hi = (long)Smax - Sq;
  p = p < 0 ? 0 : (p > hi ? hi : p);
  return (int)p;
}

template <int D, int TPW>
__launch_bounds__(PA_NW * 64)
__global__ void prefill_attn_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ kc,
    const unsigned short* __restrict__ vc, unsigned short* __restrict__ out,
    const long* __restrict__ pos_ptr, int pos_stride, long pos_host, int Hkv,
    int G, int Sq, int Smax, int ptw, long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss, long v_sb, long v_sh, long v_ss,
    long o_sb, long o_sh, long o_ss, float scale_log2) {
  constexpr int KC = D / 32;   // 32-wide chunks of the head dim (QK^T)
  constexpr int DC = D / 16;   // 16-wide output column groups (PV)
  __shared__ __attribute__((aligned(16))) unsigned short k_lds[PA_KT * D];   // K[key][d], swzD
  __shared__ __attribute__((aligned(16))) unsigned short vt_lds[D * PA_KT];  // V^T[d][key], swz32
  __shared__ __attribute__((aligned(16))) unsigned short p_lds[PA_NW * 16 * PA_KT];  // P per wave, swz32

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid % WAVE;
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int PT = ptw * PA_WQ;
  const int ptile = gridDim.x - 1 - blockIdx.x;  // longest key loops first
  const int t0 = ptile * PT;
  const int t1 = min(t0 + PT, Sq);
  const int bh = blockIdx.y;
  const int b = bh / Hkv, h = bh % Hkv;
  const int p0 = pa_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int kend = p0 + t1;    // this tile's frontier, <= Smax

  // wave tiles of this wave: tile wt is head wt % G, positions
  // [t0 + (wt / G) * 16, +16)
  const int NT = G * ptw;
  int r0[TPW], gq[TPW];
  bool act[TPW];
  pa_bf16x8 a_q[TPW][KC];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int wt = wid + t * PA_NW;
    gq[t] = wt % G;
    r0[t] = t0 + (wt / G) * PA_WQ;
    act[t] = wt < NT && r0[t] < t1;
    if (act[t]) {
      const int r = min(r0[t] + l15, Sq - 1);   // padding rows re-read the last
      const unsigned short* qp = q + (long)b * q_sb +
                                 (long)(h * G + gq[t]) * q_sh + (long)r * q_ss;
#pragma unroll
      for (int c = 0; c < KC; ++c) a_q[t][c] = pa_pack8(qp + c * 32 + lg * 8);
    } else {
#pragma unroll
      for (int c = 0; c < KC; ++c) a_q[t][c] = (pa_bf16x8)(__bf16)0.f;
    }
  }

  float m_run[TPW][4], l_run[TPW][4];
  pa_f32x4 acc_o[TPW][DC];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m_run[t][i] = -INFINITY;
      l_run[t][i] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < DC; ++d) acc_o[t][d] = (pa_f32x4)(0.f);
  }

  const unsigned short* kp = kc + (long)b * k_sb + (long)h * k_sh;
  const unsigned short* vp = vc + (long)b * v_sb + (long)h * v_sh;

  // async-STAGE split: each thread owns ONE 8-element chunk of the K and of
  // the V tile (PA_KT * D == PA_NW * 64 * 8 at D = 128; half the threads own
  // one at D = 64).  Keys at or past the frontier are staged as zeros and
  // never loaded: dead cache slots may hold anything, NaN included.
  const int st_idx = tid * 8;
  const int st_key = st_idx / D;
  const int st_col = st_idx % D;
  const bool st_own = st_idx < PA_KT * D;
  pa_bf16x8 k_reg = (pa_bf16x8)(__bf16)0.f, v_reg = (pa_bf16x8)(__bf16)0.f;

  auto stage_load = [&](int kt0) {
    if (!st_own) return;
    const int gkey = kt0 + st_key;
    if (gkey < kend) {
      k_reg = pa_pack8(kp + (long)gkey * k_ss + st_col);
      v_reg = pa_pack8(vp + (long)gkey * v_ss + st_col);
    } else {
      k_reg = (pa_bf16x8)(__bf16)0.f;
      v_reg = (pa_bf16x8)(__bf16)0.f;
    }
  };

  stage_load(0);
  unsigned short* pw = &p_lds[wid * 16 * PA_KT];

  for (int kt0 = 0; kt0 < kend; kt0 += PA_KT) {
    __syncthreads();
    if (st_own) {
      *(pa_bf16x8*)&k_lds[pa_swzD<D>(st_key, st_col)] = k_reg;
      const unsigned short* vsrc = (const unsigned short*)&v_reg;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vt_lds[pa_swz32(st_col + j, st_key)] = vsrc[j];
    }
    __syncthreads();
    if (kt0 + PA_KT < kend) stage_load(kt0 + PA_KT);

#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      // last key any row of this wave tile sees: p0 + r0 + 15.  Wave-uniform.
      if (!act[t] || kt0 > p0 + r0[t] + PA_WQ - 1) continue;

      pa_f32x4 s_acc[PA_KT / 16];
#pragma unroll
      for (int kg = 0; kg < PA_KT / 16; ++kg) {
        s_acc[kg] = (pa_f32x4)(0.f);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          pa_bf16x8 b_k =
              pa_pack8(&k_lds[pa_swzD<D>(kg * 16 + l15, c * 32 + lg * 8)]);
          s_acc[kg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_q[t][c], b_k, s_acc[kg], 0, 0, 0);
        }
      }

      // the tile crosses the diagonal if its last key is hidden from the
      // wave tile's first row; only then is the mask evaluated
      const bool diag = kt0 + PA_KT - 1 > p0 + r0[t];
#pragma unroll
      for (int kg = 0; kg < PA_KT / 16; ++kg)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) s_acc[kg][rr] *= scale_log2;
      if (diag) {
#pragma unroll
        for (int kg = 0; kg < PA_KT / 16; ++kg) {
          const int key = kt0 + kg * 16 + l15;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int lim = p0 + r0[t] + lg * 4 + rr;
            s_acc[kg][rr] = key <= lim ? s_acc[kg][rr] : -INFINITY;
          }
        }
      }

      // key 0 is visible to every row and tile 0 is never skipped, so m_new
      // is finite from the first tile on and exp2(-inf - m_new) is 0
      float alpha[4];
      float p_val[PA_KT / 16][4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float tm = s_acc[0][rr];
#pragma unroll
        for (int kg = 1; kg < PA_KT / 16; ++kg) tm = fmaxf(tm, s_acc[kg][rr]);
        tm = group16_max(tm);
        const float m_new = fmaxf(m_run[t][rr], tm);
        alpha[rr] = __builtin_amdgcn_exp2f(m_run[t][rr] - m_new);
        m_run[t][rr] = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kg = 0; kg < PA_KT / 16; ++kg) {
          const float pv = __builtin_amdgcn_exp2f(s_acc[kg][rr] - m_new);
          p_val[kg][rr] = pv;
          psum += pv;
        }
        psum = group16_sum(psum);
        l_run[t][rr] = l_run[t][rr] * alpha[rr] + psum;
      }

#pragma unroll
      for (int d = 0; d < DC; ++d)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc_o[t][d][rr] *= alpha[rr];

      // P: C layout -> A layout through this wave's own LDS slab
#pragma unroll
      for (int kg = 0; kg < PA_KT / 16; ++kg)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          pw[pa_swz32(lg * 4 + rr, kg * 16 + l15)] = f2bf(p_val[kg][rr]);

      pa_bf16x8 a_p = pa_pack8(&pw[pa_swz32(l15, lg * 8)]);
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        pa_bf16x8 b_v = pa_pack8(&vt_lds[pa_swz32(d * 16 + l15, lg * 8)]);
        acc_o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_p, b_v, acc_o[t][d], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (!act[t]) continue;
    unsigned short* op = out + (long)b * o_sb + (long)(h * G + gq[t]) * o_sh;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = r0[t] + lg * 4 + rr;
      if (row >= t1) continue;
      const float l = l_run[t][rr];
#pragma unroll
      for (int d = 0; d < DC; ++d)
        op[(long)row * o_ss + d * 16 + l15] = f2bf(acc_o[t][d][rr] / l);
    }
  }
}

void pa_check_kv(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 4 && t.stride(3) == 1,
              "prefill_attention: ", name,
              " must be 4-D bf16 CUDA with contiguous head dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr()) % 16 == 0,
              "prefill_attention: ", name,
              " must allow 16-byte loads (strides % 8, 16-byte base)");
}

}  // namespace

#pragma clang attribute pop

// Position-tile length (in 16-row wave tiles) of the launch for a problem:
// 16/G fills the 16 wave-tile slots of a workgroup with all G heads; it is
// halved while the grid would not cover the CUs, and never exceeds what Sq
// needs.  Depends on shapes and the device only, never on pos.
static int pa_choose_ptw(int G, int Sq, int BH, int cus, long forced) {
  const int need = (Sq + PA_WQ - 1) / PA_WQ;
  int ptw = std::min(std::max(1, PA_MAX_TILES / G), need);
  if (forced > 0) return (int)std::min<long>(forced, ptw);
  while (ptw > 1 && (long)BH * ((need + ptw - 1) / ptw) < cus)
    ptw = (ptw + 1) / 2;
  return ptw;
}

// out: (B, Hq, Sq, D) bf16 view (any strides, contiguous head dim), written
// in place and returned.  pos_t: optional int64 device tensor (1 or B
// elements) that overrides pos0.  pos_tile: position-tile length override in
// 16-row wave tiles (0 = auto; clamped to what G and Sq allow).
torch::Tensor prefill_attention(torch::Tensor q, torch::Tensor k_cache,
                                torch::Tensor v_cache, torch::Tensor out,
                                c10::optional<torch::Tensor> pos_t, long pos0,
                                double scale, long pos_tile) {
  pa_check_kv(q, "q");
  pa_check_kv(k_cache, "k_cache");
  pa_check_kv(v_cache, "v_cache");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 &&
              out.dim() == 4 && out.stride(3) == 1);
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  const long Sq_l = q.size(2);
  const int Hkv = k_cache.size(1);
  const long Smax_l = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "prefill_attention: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_cache.size(0) == B && k_cache.size(3) == D &&
              v_cache.size(0) == B && v_cache.size(1) == Hkv &&
              v_cache.size(2) == Smax_l && v_cache.size(3) == D,
              "prefill_attention: cache shape mismatch");
  TORCH_CHECK(out.size(0) == B && out.size(1) == Hq && out.size(2) == Sq_l &&
              out.size(3) == D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "prefill_attention: Hq % Hkv != 0");
  TORCH_CHECK(B >= 1 && Sq_l >= 1 && Smax_l >= Sq_l && Smax_l < (1L << 30),
              "prefill_attention: need 1 <= Sq <= Smax < 2^30, got Sq=", Sq_l,
              " Smax=", Smax_l);
  const int Sq = (int)Sq_l, Smax = (int)Smax_l;
  const int G = Hq / Hkv;
  TORCH_CHECK(G <= PA_MAX_G, "prefill_attention: Hq/Hkv = ", G,
              " exceeds the kernel's ", PA_MAX_G, " query heads per kv head");
  const long* pos_ptr = nullptr;
  int pos_stride = 0;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->is_cuda() && pos_t->scalar_type() == torch::kLong &&
                    pos_t->is_contiguous() &&
                    (pos_t->numel() == 1 || pos_t->numel() == B),
                "prefill_attention: pos0 tensor must be int64 CUDA with 1 or "
                "B elements");
    pos_ptr = (const long*)pos_t->data_ptr();
    pos_stride = pos_t->numel() == 1 ? 0 : 1;
  } else {
    TORCH_CHECK(pos0 >= 0 && pos0 + Sq <= Smax, "prefill_attention: pos0=",
                pos0, " with Sq=", Sq, " outside the cache (Smax=", Smax, ")");
  }

  TORCH_CHECK(pos_tile >= 0);
  const long BH = (long)B * Hkv;
  TORCH_CHECK(BH <= 65535, "prefill_attention: B*Hkv = ", BH,
              " exceeds the grid's y extent");
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int ptw = pa_choose_ptw(G, Sq, (int)BH, cus, pos_tile);
  const int ntile = (Sq + ptw * PA_WQ - 1) / (ptw * PA_WQ);
  const int tpw = (G * ptw + PA_NW - 1) / PA_NW;   // 1 or 2
  TORCH_CHECK(tpw >= 1 && tpw <= 2);

  const float scale_log2 = (float)(scale * 1.4426950408889634);
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid((unsigned)ntile, (unsigned)BH), block(PA_NW * 64);
  const unsigned short* qp = (const unsigned short*)q.data_ptr();
  const unsigned short* kp = (const unsigned short*)k_cache.data_ptr();
  const unsigned short* vp = (const unsigned short*)v_cache.data_ptr();
  unsigned short* op = (unsigned short*)out.data_ptr();
#define PA_LAUNCH(D_, T_)                                                     \
  hipLaunchKernelGGL((prefill_attn_kernel<D_, T_>), grid, block, 0, stream,   \
                     qp, kp, vp, op, pos_ptr, pos_stride, pos0, Hkv, G, Sq,   \
                     Smax, ptw, q.stride(0), q.stride(1), q.stride(2),        \
                     k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), \
                     v_cache.stride(0), v_cache.stride(1), v_cache.stride(2), \
                     out.stride(0), out.stride(1), out.stride(2), scale_log2)
  if (D == 64) {
    if (tpw == 1) PA_LAUNCH(64, 1); else PA_LAUNCH(64, 2);
  } else {
    if (tpw == 1) PA_LAUNCH(128, 1); else PA_LAUNCH(128, 2);
  }
#undef PA_LAUNCH
  HIP_CHECK_LAST();
  return out;
}
