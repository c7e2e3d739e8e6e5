// What the split-KV decode-attention kernels share (decode_attn.hip over a
// bf16 cache, decode_attn_paged.hip over a paged bf16 cache,
// decode_attn_fp8.hip over an fp8 cache): the DPP lane-group reduction, the
// clamped position read, the split choice and the body of the combine
// launch.  The body of the first launch of the two bf16 kernels is shared as
// text, in decode_attn_body.inc.
#pragma once

#include <algorithm>

#include "common.h"

#define DA_BLOCK 256
#define DA_WAVES (DA_BLOCK / WAVE)
#define DA_MAX_M 16
#define DA_MAX_IDS 4096   // page ids a paged workgroup keeps in LDS (16 KB)

typedef short da_sv2 __attribute__((ext_vector_type(2)));

template <int CTRL>
DEVINL float da_dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF,
                                            0xF, false);
  return v + __int_as_float(t);
}

// all-reduce sum over aligned groups of LPK (4, 8 or 16) lanes, VALU only
template <int LPK>
DEVINL float da_group_sum(float v) {
  if (LPK == 16) v = da_dpp_add<0x140>(v);  // row_mirror: i <-> 15-i
  if (LPK >= 8) v = da_dpp_add<0x141>(v);   // row_half_mirror: i <-> 7-i
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

// Body of the second launch (grid (B*Hkv, M), D threads): merge the
// per-split partials of one (batch, kv head, row).  Only splits that start
// below the valid length were written; the rest of the workspace is never
// read.
template <int D>
DEVINL void da_combine(const float* __restrict__ part_acc,
                       const float* __restrict__ part_ml,
                       ushort* __restrict__ out,
                       const long* __restrict__ pos_ptr, int pos_stride,
                       long pos_host, int Hkv, int G, int Sq, int Smax,
                       int chunk, int nsplit, int MT, long o_sb, long o_sh,
                       long o_ss) {
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

// KV chunk length per workgroup, a multiple of 64: from Smax and the CU
// count only, so a captured grid stays valid (split_kv > 0 overrides)
static inline int da_choose_chunk(int Smax, int BH, long split_kv, int cus) {
  if (split_kv > 0)
    return (int)std::min<long>((split_kv + 63) / 64 * 64, 1L << 30);
  const int want = std::max(1, (2 * cus + BH - 1) / BH);
  return ((Smax + want - 1) / want + 63) / 64 * 64;
}

// The same for a paged cache: a whole number of pages, a multiple of
// max(64, page), and at most DA_MAX_IDS pages (then nsplit grows instead)
static inline int da_choose_chunk_paged(int Smax, int BH, long split_kv,
                                        int cus, int page) {
  const long m = std::max(64, page);
  const long c = da_choose_chunk(Smax, BH, split_kv, cus);
  return (int)std::min<long>((c + m - 1) / m * m, (long)DA_MAX_IDS * page);
}
