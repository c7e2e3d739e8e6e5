// Fused temperature / top-k / top-p sampling for gfx950 (wave64): one launch,
// one workgroup of 16 waves per logits row, the row re-read from L2 on each
// pass; nothing of size V is written anywhere and the row is never sorted.
//
// Keys.  Every logit becomes an order-preserving integer key (16 bits for
// bf16, 32 for fp32; -0 folds onto +0), read 8 bits at a time from the top.
// Selection runs on the keys of x, not on x / T.
//
// Weights.  w = exp2((x - xmax) * log2(e) / T) is turned into the integer
// q = trunc(w * 2^40) and every sum that decides an outcome is a sum of q in
// 64-bit integers: integer addition is associative, so the LDS atomics that
// build the histograms and the shuffle trees that reduce tiles give the same
// bits on every run, in any order.  Elements with one key have one q.  A row
// of 2^18 elements sums to below 2^58; what the truncation drops is below
// V * 2^-40 of the largest weight.
//
// Passes over the row (D = key bytes: 2 for bf16, 4 for fp32):
//   1      the largest key, and with top-k the count histogram of the top
//          digit (256 bins, REP replicas by lane to spread the atomics)
//   top-k  D-1 passes: the count (and, when top-p follows, mass) histogram of
//          the next digit under the prefix found so far; a suffix scan by
//          wave 0 picks the bin of the k-th largest.  The end is the exact
//          k-th key t, the number above it and the ties at t to admit.  The
//          first of these passes also takes the mass histogram of the top
//          digit over the whole row, which the top-p descent starts from.
//   top-p  D-1 passes (plus one for the top digit when top-k is off): the same
//          descent on mass: the bin where the mass from the top reaches
//          top_p * mass(K).  The end is the exact key t2 of the last nucleus
//          member and m = ceil(rest / q(t2)) ties to admit.
//   draw   one pass: the row as tiles of 64 vectors (one wave iteration);
//          per tile the mass above the cut and the ties at it, by shuffle
//          trees.  One thread per tile admits ties in index order from a block
//          scan of the tie counts, a second block scan gives the running mass
//          in index order and C_last, and the tile that holds
//          floor(u * C_last) is re-read by wave 0, which scans its 64 vectors
//          and walks one of them to the token.
//
// Rows start on any element boundary: vectors are the 16-byte aligned pieces
// that cover the row, the first and last of them read element by element
// inside [0, V), all others with one 16-byte load.
//
// Out of contract (a row of -inf, NaN): the result is some index in
// [0, V - 1]; nothing is read or written outside the buffers.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int SB = 1024;              // threads per row
constexpr int SNW = SB / WAVE;
constexpr int NBIN = 256;
constexpr int REP = 4;                // histogram replicas, by lane
constexpr int MAX_TILES = SB;         // one thread per tile in the draw
constexpr float QSCALE = 1099511627776.f;        // 2^40
constexpr float LOG2E = 1.4426950408889634f;

template <int KB> struct KeyT {
  static constexpr unsigned SIGN = 1u << (KB - 1);
  static constexpr unsigned FULL = KB == 32 ? 0xffffffffu : ((1u << (KB % 32)) - 1u);
  static constexpr int VEC = 128 / KB;           // elements per 16 bytes
  static constexpr int ESIZE = KB / 8;
  static constexpr int D = KB / 8;               // digits
};

template <int KB> DEVINL unsigned key_of(unsigned raw) {
  typedef KeyT<KB> K;
  if ((raw & (K::SIGN - 1u)) == 0u) raw = 0u;
  return (raw & K::SIGN) ? (~raw & K::FULL) : (raw | K::SIGN);
}

template <int KB> DEVINL float val_of_key(unsigned key) {
  typedef KeyT<KB> K;
  const unsigned raw = (key & K::SIGN) ? (key ^ K::SIGN) : (~key & K::FULL);
  return __uint_as_float(KB == 16 ? raw << 16 : raw);
}

template <int KB> DEVINL u64 q_of_key(unsigned key, float xmax, float scale) {
  const float w = __builtin_amdgcn_exp2f((val_of_key<KB>(key) - xmax) * scale);
  // w in [0, 1] in contract; the clamp keeps the conversion defined for NaN
  return (u64)fminf(fmaxf(w * QSCALE, 0.f), QSCALE);
}

// The row as 16-byte aligned vectors: vector j holds elements
// j * VEC - off + (0..VEC-1), those inside [0, V) are valid.
template <int KB> struct Row {
  const char* base;      // first element
  int off, V, NV;
};

// keys of vector j; returns the mask of valid elements
template <int KB>
DEVINL unsigned load_keys(const Row<KB>& r, int j, unsigned* keys) {
  typedef KeyT<KB> K;
  const int e0 = j * K::VEC - r.off;
  if (e0 >= 0 && e0 + K::VEC <= r.V) {
    const uint4 v = *(const uint4*)(r.base + (long)e0 * K::ESIZE);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < K::VEC; ++e)
      keys[e] = key_of<KB>(KB == 16 ? (w[e >> 1] >> (16 * (e & 1))) & 0xffffu
                                    : w[e & 3]);
    return (1u << K::VEC) - 1u;
  }
  unsigned mask = 0u;
#pragma unroll
  for (int e = 0; e < K::VEC; ++e) {
    const int i = e0 + e;
    keys[e] = 0u;
    if (i >= 0 && i < r.V) {
      const unsigned raw = KB == 16
          ? (unsigned)((const unsigned short*)r.base)[i]
          : ((const unsigned*)r.base)[i];
      keys[e] = key_of<KB>(raw);
      mask |= 1u << e;
    }
  }
  return mask;
}

DEVINL u64 wave_scan_incl64(u64 v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const u64 t = __shfl_up(v, off, WAVE);
    if (lane >= off) v += t;
  }
  return v;
}

DEVINL u64 wave_sum64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// exclusive scan over the block in thread order; *total = the block sum
DEVINL u64 block_scan_excl64(u64 v, u64* wtot, u64* total) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const u64 incl = wave_scan_incl64(v, lane);
  if (lane == WAVE - 1) wtot[w] = incl;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SNW; ++i) {
    const u64 t = wtot[i];
    base += i < w ? t : 0ull;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// one digit of one prefix: elements with (key & mask) == bits add to bin
// (key >> shift) & 255 of histogram `slot`
struct Slot { unsigned mask, bits; int shift; bool cnt, mass; };

template <int KB> DEVINL Slot slot_of(unsigned prefix, int lvl, bool cnt,
                                      bool mass) {
  Slot s;
  s.shift = KB - 8 * (lvl + 1);
  s.mask = lvl == 0 ? 0u : (KeyT<KB>::FULL >> (s.shift + 8)) << (s.shift + 8);
  s.bits = lvl == 0 ? 0u : prefix << (s.shift + 8);
  s.cnt = cnt;
  s.mass = mass;
  return s;
}

struct Lds {
  unsigned cnt[2][NBIN * REP];
  u64 mass[2][NBIN * REP];
  u64 mass0[NBIN];          // top-digit masses of the whole row
  u64 hm[NBIN];             // merged histogram under the current prefix
  unsigned hc[NBIN];
  u64 tile_mass[MAX_TILES];
  unsigned tile_ties[MAX_TILES];
  u64 wtot[SNW];
  unsigned wmax[SNW];
  int bin;
  u64 above;
  int tile;
  u64 tile_excl;
  unsigned tile_tb;
};

template <int KB>
DEVINL unsigned first_pass(const Row<KB>& r, bool count, Lds& s) {
  typedef KeyT<KB> K;
  const int rep = threadIdx.x & (REP - 1);
  unsigned best = 0u;
  for (int j = threadIdx.x; j < r.NV; j += SB) {
    unsigned keys[K::VEC];
    const unsigned m = load_keys<KB>(r, j, keys);
#pragma unroll
    for (int e = 0; e < K::VEC; ++e) {
      if (!((m >> e) & 1u)) continue;
      best = keys[e] > best ? keys[e] : best;
      if (count) atomicAdd(&s.cnt[0][(keys[e] >> (KB - 8)) * REP + rep], 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(best, off, WAVE);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) s.wmax[threadIdx.x / WAVE] = best;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SNW; ++i) best = s.wmax[i] > best ? s.wmax[i] : best;
  return best;
}

template <int KB>
DEVINL void add_to(const Slot& a, int slot, unsigned key, u64 q, int rep,
                   Lds& s) {
  const int d = (key >> a.shift) & 255;
  if (a.cnt) atomicAdd(&s.cnt[slot][d * REP + rep], 1u);
  if (a.mass && q) atomicAdd(&s.mass[slot][d * REP + rep], q);
}

template <int KB>
DEVINL void hist_pass(const Row<KB>& r, const Slot a, const Slot b, bool use_b,
                      float xmax, float scale, Lds& s) {
  typedef KeyT<KB> K;
  const int rep = threadIdx.x & (REP - 1);
  const bool any_mass = a.mass || (use_b && b.mass);
  for (int j = threadIdx.x; j < r.NV; j += SB) {
    unsigned keys[K::VEC];
    const unsigned m = load_keys<KB>(r, j, keys);
#pragma unroll
    for (int e = 0; e < K::VEC; ++e) {
      const unsigned key = keys[e];
      const bool ok = (m >> e) & 1u;
      const bool ma = ok && (key & a.mask) == a.bits;
      const bool mb = ok && use_b && (key & b.mask) == b.bits;
      if (!(ma || mb)) continue;
      const u64 q = any_mass ? q_of_key<KB>(key, xmax, scale) : 0ull;
      if (ma) add_to<KB>(a, 0, key, q, rep, s);
      if (mb) add_to<KB>(b, 1, key, q, rep, s);
    }
  }
}

// replicas of histogram `slot` -> hc, hm; the replicas are left zeroed
DEVINL void merge_hist(int slot, Lds& s) {
  __syncthreads();
  if (threadIdx.x < NBIN) {
    unsigned c = 0u;
    u64 q = 0ull;
#pragma unroll
    for (int i = 0; i < REP; ++i) {
      c += s.cnt[slot][threadIdx.x * REP + i];
      q += s.mass[slot][threadIdx.x * REP + i];
      s.cnt[slot][threadIdx.x * REP + i] = 0u;
      s.mass[slot][threadIdx.x * REP + i] = 0ull;
    }
    s.hc[threadIdx.x] = c;
    s.hm[threadIdx.x] = q;
  }
  __syncthreads();
}

// The highest bin b with sum(v[b..255]) >= target, and sum(v[b+1..255]), by
// wave 0: lane l scans bins 255 - 4l .. 252 - 4l.  v is hm (hc when null).
// A target above the total is cut to it.
DEVINL void find_bin(const u64* hm, const unsigned* hc, u64 target, Lds& s,
                     int* bin, u64* above) {
  if (threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    u64 v[4], sum = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = NBIN - 1 - (4 * lane + i);
      v[i] = hm ? hm[b] : (u64)hc[b];
      sum += v[i];
    }
    const u64 incl = wave_scan_incl64(sum, lane);
    const u64 total = __shfl(incl, WAVE - 1, WAVE);
    target = target > total ? total : target;
    u64 cum = incl - sum, fa = 0ull;
    int fb = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (fb < 0 && target > 0ull && cum + v[i] >= target) {
        fb = NBIN - 1 - (4 * lane + i);
        fa = cum;
      }
      cum += v[i];
    }
    const u64 bal = __ballot(fb >= 0);
    if (bal == 0ull) {
      if (lane == 0) { s.bin = 0; s.above = 0ull; }
    } else if (lane == __ffsll((long long)bal) - 1) {
      s.bin = fb;
      s.above = fa;
    }
  }
  __syncthreads();
  *bin = s.bin;
  *above = s.above;
  __syncthreads();
}

// sum of h[b+1..255] (b = -1: everything)
DEVINL u64 above_of(const u64* h, int b, Lds& s) {
  if (threadIdx.x < WAVE) {
    u64 sum = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = 4 * threadIdx.x + i;
      sum += d > b ? h[d] : 0ull;
    }
    sum = wave_sum64(sum);
    if (threadIdx.x == 0) s.above = sum;
  }
  __syncthreads();
  const u64 out = s.above;
  __syncthreads();
  return out;
}

template <int KB>
__global__ __launch_bounds__(SB) void sample_kernel(
    const char* __restrict__ logits, long row_bytes, int V,
    const float* __restrict__ u, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p,
    long long* __restrict__ out) {
  typedef KeyT<KB> K;
  __shared__ Lds s;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int row = blockIdx.x;

  Row<KB> r;
  r.base = logits + (long)row * row_bytes;
  r.off = (int)(((uintptr_t)r.base & 15u) / K::ESIZE);
  r.V = V;
  r.NV = (r.off + V + K::VEC - 1) / K::VEC;
  const int ntiles = (r.NV + WAVE - 1) / WAVE;

  const float T = fmaxf(temperature[row], 1e-5f);
  const int k = top_k[row];
  const float tp = top_p[row];
  const bool k_act = k > 0 && k < V;
  const bool p_act = tp < 1.f;

  for (int i = tid; i < NBIN * REP; i += SB) {
    s.cnt[0][i] = s.cnt[1][i] = 0u;
    s.mass[0][i] = s.mass[1][i] = 0ull;
  }
  s.tile_mass[tid] = 0ull;
  s.tile_ties[tid] = 0u;
  __syncthreads();

  const unsigned kmax = first_pass<KB>(r, k_act, s);
  const float xmax = val_of_key<KB>(kmax);
  const float scale = LOG2E / T;

  // the cut: keys above tc are kept, and the first mc keys equal to tc
  unsigned tc = 0u, mc = 0xffffffffu;
  unsigned tk = 0u, mk = 0xffffffffu;
  u64 massK = 0ull;
  int bin;
  u64 above;

  if (k_act) {
    merge_hist(0, s);
    find_bin(nullptr, s.hc, (u64)k, s, &bin, &above);
    unsigned krem = (unsigned)k - (unsigned)above;
    unsigned pref = (unsigned)bin;
    u64 mgt = 0ull;
    for (int lvl = 1; lvl < K::D; ++lvl) {
      const bool use_b = p_act && lvl == 1;
      hist_pass<KB>(r, slot_of<KB>(pref, lvl, true, p_act),
                    slot_of<KB>(0u, 0, false, true), use_b, xmax, scale, s);
      if (use_b) {
        merge_hist(1, s);
        if (tid < NBIN) s.mass0[tid] = s.hm[tid];
        __syncthreads();
        mgt += above_of(s.mass0, (int)pref, s);
      }
      merge_hist(0, s);
      find_bin(nullptr, s.hc, (u64)krem, s, &bin, &above);
      krem -= (unsigned)above;
      if (p_act) mgt += above_of(s.hm, bin, s);
      pref = (pref << 8) | (unsigned)bin;
    }
    tk = pref;
    mk = krem > 0u ? krem : 1u;
    massK = mgt + (u64)mk * q_of_key<KB>(tk, xmax, scale);
    tc = tk;
    mc = mk;
  }

  if (p_act) {
    if (!k_act) {
      hist_pass<KB>(r, slot_of<KB>(0u, 0, false, true),
                    slot_of<KB>(0u, 0, false, false), false, xmax, scale, s);
      merge_hist(0, s);
      if (tid < NBIN) s.mass0[tid] = s.hm[tid];
      __syncthreads();
      massK = above_of(s.mass0, -1, s);
    }
    const double pd = ceil((double)fmaxf(tp, 0.f) * (double)massK);
    u64 prem = (u64)pd;
    prem = prem > massK ? massK : prem;
    prem = prem < 1ull ? 1ull : prem;
    find_bin(s.mass0, nullptr, prem, s, &bin, &above);
    prem -= above;
    unsigned pref = (unsigned)bin;
    for (int lvl = 1; lvl < K::D; ++lvl) {
      hist_pass<KB>(r, slot_of<KB>(pref, lvl, true, true),
                    slot_of<KB>(0u, 0, false, false), false, xmax, scale, s);
      merge_hist(0, s);
      find_bin(s.hm, nullptr, prem, s, &bin, &above);
      prem -= above;
      pref = (pref << 8) | (unsigned)bin;
    }
    const unsigned cnt2 = s.hc[bin];
    const u64 q2 = q_of_key<KB>(pref, xmax, scale);
    u64 m = q2 ? (prem + q2 - 1ull) / q2 : 1ull;
    m = m < 1ull ? 1ull : m;
    m = m > (u64)cnt2 && cnt2 > 0u ? (u64)cnt2 : m;
    unsigned t2 = pref;
    if (k_act && t2 < tk) { t2 = tk; m = mk; }
    if (k_act && t2 == tk && m > (u64)mk) m = mk;
    tc = t2;
    mc = (unsigned)m;
    __syncthreads();
  }

  // ---- draw: tiles of 64 vectors, tile = (iteration, wave)
  const u64 qc = q_of_key<KB>(tc, xmax, scale);
  for (int j0 = wave * WAVE; j0 < r.NV; j0 += SB) {
    const int j = j0 + lane;
    u64 gt = 0ull;
    unsigned ties = 0u;
    if (j < r.NV) {
      unsigned keys[K::VEC];
      const unsigned m = load_keys<KB>(r, j, keys);
#pragma unroll
      for (int e = 0; e < K::VEC; ++e) {
        if (!((m >> e) & 1u)) continue;
        if (keys[e] > tc) gt += q_of_key<KB>(keys[e], xmax, scale);
        ties += keys[e] == tc ? 1u : 0u;
      }
    }
    gt = wave_sum64(gt);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ties += __shfl_xor(ties, off, WAVE);
    if (lane == 0) {
      s.tile_mass[j0 / WAVE] = gt;
      s.tile_ties[j0 / WAVE] = ties;
    }
  }
  if (tid == 0) s.tile = -1;
  __syncthreads();

  {
    const unsigned ties = s.tile_ties[tid];
    u64 total;
    const u64 tb = block_scan_excl64((u64)ties, s.wtot, &total);
    const u64 room = (u64)mc > tb ? (u64)mc - tb : 0ull;
    const u64 adm = room < (u64)ties ? room : (u64)ties;
    const u64 mine = s.tile_mass[tid] + adm * qc;
    const u64 excl = block_scan_excl64(mine, s.wtot, &total);
    const u64 target = (u64)floor((double)u[row] * (double)total);
    if (tid < ntiles && excl <= target && target < excl + mine) {
      s.tile = tid;
      s.tile_excl = excl;
      s.tile_tb = (unsigned)tb;
    }
    __syncthreads();
    const int tile = s.tile;
    if (tile < 0) {                     // out of contract: no mass at all
      if (tid == 0) out[row] = 0;
      return;
    }
    if (wave != 0) return;
    const int j = tile * WAVE + lane;
    unsigned keys[K::VEC];
    unsigned m = 0u;
    if (j < r.NV) m = load_keys<KB>(r, j, keys);
    unsigned lt = 0u;
#pragma unroll
    for (int e = 0; e < K::VEC; ++e)
      lt += ((m >> e) & 1u) && keys[e] == tc ? 1u : 0u;
    unsigned rank = lt;                 // ties of the tile before this lane
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const unsigned t = __shfl_up(rank, off, WAVE);
      if (lane >= off) rank += t;
    }
    rank = rank - lt + s.tile_tb;
    u64 q[K::VEC], lsum = 0ull;
#pragma unroll
    for (int e = 0; e < K::VEC; ++e) {
      q[e] = 0ull;
      if (!((m >> e) & 1u)) continue;
      if (keys[e] > tc) q[e] = q_of_key<KB>(keys[e], xmax, scale);
      else if (keys[e] == tc) q[e] = rank++ < mc ? qc : 0ull;
      lsum += q[e];
    }
    u64 cum = wave_scan_incl64(lsum, lane) - lsum + s.tile_excl;
    if (cum <= target && target < cum + lsum) {
      int tok = 0;
      bool done = false;
#pragma unroll
      for (int e = 0; e < K::VEC; ++e) {
        cum += q[e];
        if (!done && q[e] && cum > target) {
          tok = j * K::VEC - r.off + e;
          done = true;
        }
      }
      tok = tok < 0 ? 0 : (tok > V - 1 ? V - 1 : tok);
      out[row] = tok;
    }
  }
}

}  // namespace

// logits (B, V) bf16 | fp32 with unit last stride; u, temperature, top_p (B,)
// fp32; top_k (B,) int32; out (B,) int64 contiguous.  Returns out.
torch::Tensor sample_logits(torch::Tensor logits, torch::Tensor u,
                            torch::Tensor temperature, torch::Tensor top_k,
                            torch::Tensor top_p, torch::Tensor out) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              (logits.scalar_type() == torch::kBFloat16 ||
               logits.scalar_type() == torch::kFloat),
              "sample_logits: logits must be a (B, V) bf16 or fp32 CUDA "
              "tensor");
  const long B = logits.size(0), V = logits.size(1);
  const bool bf = logits.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(V >= 1 && (V == 1 || logits.stride(1) == 1),
              "sample_logits: logits need stride(-1) == 1");
  TORCH_CHECK(B <= 1 || logits.stride(0) >= V,
              "sample_logits: logits rows overlap");
  // one thread per tile of 64 vectors in the draw
  const long vmax = (long)MAX_TILES * WAVE * (bf ? 8 : 4) - 8;
  TORCH_CHECK(V <= vmax, "sample_logits: V = ", V, " above ", vmax);
  for (const torch::Tensor* t : {&u, &temperature, &top_p})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat &&
                t->dim() == 1 && t->size(0) == B && t->is_contiguous() &&
                t->device() == logits.device(),
                "sample_logits: u, temperature and top_p must be contiguous "
                "(B,) fp32 tensors on the logits' device");
  TORCH_CHECK(top_k.is_cuda() && top_k.scalar_type() == torch::kInt &&
              top_k.dim() == 1 && top_k.size(0) == B &&
              top_k.is_contiguous() && top_k.device() == logits.device(),
              "sample_logits: top_k must be a contiguous (B,) int32 tensor "
              "on the logits' device");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kLong &&
              out.dim() == 1 && out.size(0) == B && out.is_contiguous() &&
              out.device() == logits.device(),
              "sample_logits: out must be a contiguous (B,) int64 tensor on "
              "the logits' device");
  if (B == 0) return out;
  TORCH_CHECK(B < (1L << 31), "sample_logits: B too large");
  auto stream = at::cuda::getCurrentHIPStream();
  const long row_bytes = (B > 1 ? logits.stride(0) : V) * (bf ? 2 : 4);
  const char* lp = (const char*)logits.data_ptr();
  if (bf) {
    hipLaunchKernelGGL(sample_kernel<16>, dim3((unsigned)B), dim3(SB), 0,
                       stream, lp, row_bytes, (int)V, u.data_ptr<float>(),
                       temperature.data_ptr<float>(), top_k.data_ptr<int>(),
                       top_p.data_ptr<float>(),
                       (long long*)out.data_ptr<int64_t>());
  } else {
    hipLaunchKernelGGL(sample_kernel<32>, dim3((unsigned)B), dim3(SB), 0,
                       stream, lp, row_bytes, (int)V, u.data_ptr<float>(),
                       temperature.data_ptr<float>(), top_k.data_ptr<int>(),
                       top_p.data_ptr<float>(),
                       (long long*)out.data_ptr<int64_t>());
  }
  HIP_CHECK_LAST();
  return out;
}
