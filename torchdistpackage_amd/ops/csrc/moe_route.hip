// Fused MoE token routing for gfx950 (wave64): a stable counting sort that
// turns the router's (N, k) expert ids into a destination row per (token,
// slot) entry, and the two row kernels that move tokens with it.
//
//   plan      dest[t, j] = row of entry (t, j) in the buffer sorted by expert,
//             stable in the flat index t*k + j; counts (E,), offs (E+1,)
//   scatter   out[dest[t, j]] = x[t]               (dispatch forward)
//             out[dest[t, j]] = g[t, j] * x[t]     (combine backward, which
//             also forms dgates[t, j] = x[t] . y[dest[t, j]] in the same pass)
//   gather    out[t] = sum_j g[t, j] * y[dest[t, j]]   (combine forward;
//             without gates the dispatch backward)
//
// Plan.  Entries are cut into contiguous chunks of MOE_PLAN_CHUNK, one
// workgroup each.  Launch A: an LDS histogram per chunk -> block_hist[c][E].
// Launch B (one workgroup): an exclusive scan of block_hist over the chunks
// for every expert (a wave per expert, 64 chunks per step), then a scan of
// the expert totals -> counts, offs.  Launch C: every chunk is read again in
// rounds of one entry per thread.  The rank of an entry among the entries of
// its expert is (entries of earlier rounds) + (entries of earlier waves of
// this round, from per-wave LDS histograms written by one leader lane per
// expert with a plain store) + (lower lanes of the wave with the same expert,
// by one ballot per id bit).  No atomics take part in the ranking, so the
// order is the flat index.  N*k <= MOE_PLAN_CHUNK runs all three phases in
// one workgroup and one launch.  Every size comes from host values (N*k, E):
// nothing is read back, the call captures into a hipGraph.
//
// Row kernels.  One wave per token row, four rows per workgroup; the lanes
// stride the row in 16-byte pieces (D/8 pieces over 64 lanes).  The k
// destination rows and gates of a token sit in registers; the gather issues
// its k loads of a piece before the fp32 arithmetic and stores once.  The
// dgates dots are reduced across the wave by shuffles.  No LDS, no atomics.
//
// Bounds: expert ids are clamped to [0, E-1] and every dest value to
// [0, rows-1] before they index anything, so stale indices give wrong
// answers, never an access outside the buffers.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "moe_route.h"

namespace {

constexpr int PLAN_BLOCK = 512;
constexpr int PLAN_NW = PLAN_BLOCK / WAVE;
static_assert(MOE_ROUTE_MAX_E <= PLAN_BLOCK, "one thread per expert column");
static_assert(MOE_PLAN_CHUNK % PLAN_BLOCK == 0, "whole rounds per chunk");

DEVINL int plan_id(const void* ids, int ids64, long i, int E) {
  long v = ids64 ? (long)((const long long*)ids)[i]
                 : (long)((const int*)ids)[i];
  v = v < 0 ? 0 : v;
  return (int)(v > E - 1 ? E - 1 : v);
}

// inclusive scan over the 64 lanes of a wave
DEVINL int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int u = __shfl_up(v, off, WAVE);
    if (lane >= off) v += u;
  }
  return v;
}

// Wave 0: counts[e] = tot[e], offs = exclusive scan of tot with the total at
// offs[E]; `excl` (LDS, may be null) receives the exclusive scan as well.
// tot and excl may alias.
DEVINL void plan_offsets(int* tot, int E, long long* counts, long long* offs,
                         int* excl) {
  if (threadIdx.x >= WAVE) return;
  const int lane = threadIdx.x;
  int carry = 0;
  for (int e0 = 0; e0 < E; e0 += WAVE) {
    const int e = e0 + lane;
    const int v = e < E ? tot[e] : 0;
    const int s = wave_scan_incl(v, lane);
    if (e < E) {
      counts[e] = v;
      offs[e] = carry + s - v;
      if (excl) excl[e] = carry + s - v;
    }
    carry += __shfl(s, WAVE - 1, WAVE);
  }
  if (lane == 0) offs[E] = carry;
}

// Entries [lo, hi) of one workgroup, PLAN_BLOCK per round.  running[e] holds
// the destination row of the next entry of expert e and is advanced round by
// round; whist must arrive zeroed.
DEVINL void plan_rank(const void* ids, int ids64, long lo, long hi, int E,
                      int nbits, int* running,
                      int (*whist)[MOE_ROUTE_MAX_E], int* __restrict__ dest) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long r0 = lo; r0 < hi; r0 += PLAN_BLOCK) {
    const long i = r0 + threadIdx.x;
    const bool valid = i < hi;
    const int e = valid ? plan_id(ids, ids64, i, E) : 0;
    // lanes of this wave that hold the same expert
    unsigned long long same = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
      const int bit = (e >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const int rank = __popcll(same & below);
    if (valid && rank == 0) whist[w][e] = __popcll(same);
    __syncthreads();
    if (valid) {
      int d = running[e] + rank;
      for (int u = 0; u < w; ++u) d += whist[u][e];
      dest[i] = d;
    }
    __syncthreads();
    if ((int)threadIdx.x < E) {
      int s = 0;
#pragma unroll
      for (int u = 0; u < PLAN_NW; ++u) {
        s += whist[u][threadIdx.x];
        whist[u][threadIdx.x] = 0;
      }
      running[threadIdx.x] += s;
    }
    __syncthreads();
  }
}

DEVINL void plan_zero(int* a, int n) {
  for (int i = threadIdx.x; i < n; i += PLAN_BLOCK) a[i] = 0;
}

__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_hist_kernel(
    const void* __restrict__ ids, int ids64, long n, int E,
    int* __restrict__ block_hist) {
  __shared__ int hist[MOE_ROUTE_MAX_E];
  plan_zero(hist, MOE_ROUTE_MAX_E);
  __syncthreads();
  const long lo = (long)blockIdx.x * MOE_PLAN_CHUNK;
  const long hi = lo + MOE_PLAN_CHUNK < n ? lo + MOE_PLAN_CHUNK : n;
  for (long i = lo + threadIdx.x; i < hi; i += PLAN_BLOCK)
    atomicAdd(&hist[plan_id(ids, ids64, i, E)], 1);
  __syncthreads();
  if ((int)threadIdx.x < E)
    block_hist[(long)blockIdx.x * E + threadIdx.x] = hist[threadIdx.x];
}

// block_hist (nchunks, E) in: entries per (chunk, expert); out: entries of
// the expert in earlier chunks.
__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_scan_kernel(
    int* __restrict__ block_hist, int nchunks, int E,
    long long* __restrict__ counts, long long* __restrict__ offs) {
  __shared__ int tot[MOE_ROUTE_MAX_E];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  for (int e = w; e < E; e += PLAN_NW) {
    int carry = 0;
    for (int c0 = 0; c0 < nchunks; c0 += WAVE) {
      const int c = c0 + lane;
      const int v = c < nchunks ? block_hist[(long)c * E + e] : 0;
      const int s = wave_scan_incl(v, lane);
      if (c < nchunks) block_hist[(long)c * E + e] = carry + s - v;
      carry += __shfl(s, WAVE - 1, WAVE);
    }
    if (lane == 0) tot[e] = carry;
  }
  __syncthreads();
  plan_offsets(tot, E, counts, offs, nullptr);
}

__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_rank_kernel(
    const void* __restrict__ ids, int ids64, long n, int E, int nbits,
    const int* __restrict__ base, const long long* __restrict__ offs,
    int* __restrict__ dest) {
  __shared__ int running[MOE_ROUTE_MAX_E];
  __shared__ int whist[PLAN_NW][MOE_ROUTE_MAX_E];
  plan_zero(&whist[0][0], PLAN_NW * MOE_ROUTE_MAX_E);
  if ((int)threadIdx.x < E)
    running[threadIdx.x] =
        (int)offs[threadIdx.x] + base[(long)blockIdx.x * E + threadIdx.x];
  __syncthreads();
  const long lo = (long)blockIdx.x * MOE_PLAN_CHUNK;
  const long hi = lo + MOE_PLAN_CHUNK < n ? lo + MOE_PLAN_CHUNK : n;
  plan_rank(ids, ids64, lo, hi, E, nbits, running, whist, dest);
}

// n <= MOE_PLAN_CHUNK: histogram, offsets and ranks in one workgroup
__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_small_kernel(
    const void* __restrict__ ids, int ids64, long n, int E, int nbits,
    long long* __restrict__ counts, long long* __restrict__ offs,
    int* __restrict__ dest) {
  __shared__ int running[MOE_ROUTE_MAX_E];
  __shared__ int whist[PLAN_NW][MOE_ROUTE_MAX_E];
  plan_zero(&whist[0][0], PLAN_NW * MOE_ROUTE_MAX_E);
  plan_zero(running, MOE_ROUTE_MAX_E);
  __syncthreads();
  for (long i = threadIdx.x; i < n; i += PLAN_BLOCK)
    atomicAdd(&running[plan_id(ids, ids64, i, E)], 1);
  __syncthreads();
  plan_offsets(running, E, counts, offs, running);
  __syncthreads();
  plan_rank(ids, ids64, 0, n, E, nbits, running, whist, dest);
}

// ----------------------------------------------------------- row kernels

constexpr int ROW_BLOCK = 256;
constexpr int ROWS_PER_WG = ROW_BLOCK / WAVE;

DEVINL void unpack8(const uint4& v, float* f) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

DEVINL uint4 pack8(const float* f) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = (unsigned)f2bf(f[2 * i]) | ((unsigned)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// first piece of the row that dest[t, j] names, clamped into the M-row buffer
DEVINL long row_piece0(const int* __restrict__ dest, long e, long M, int P) {
  long d = dest[e];
  d = d < 0 ? 0 : d;
  d = d > M - 1 ? M - 1 : d;
  return d * P;
}

// out (N rows) [t] = sum_j g[t, j] * y (M rows) [dest[t, j]], ascending j,
// fp32, one rounding.  P = D/8 pieces per row.
template <int K, bool GATED>
__global__ __launch_bounds__(ROW_BLOCK) void moe_gather_kernel(
    const uint4* __restrict__ y, const int* __restrict__ dest,
    const float* __restrict__ gates, uint4* __restrict__ out, long N, int P,
    long M) {
  const long t = (long)blockIdx.x * ROWS_PER_WG + threadIdx.x / WAVE;
  if (t >= N) return;
  const int lane = threadIdx.x & (WAVE - 1);
  long src[K];
  float g[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    src[j] = row_piece0(dest, t * K + j, M, P);
    g[j] = GATED ? gates[t * K + j] : 1.f;
  }
  for (int p = lane; p < P; p += WAVE) {
    uint4 v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = y[src[j] + p];
    if (K == 1 && !GATED) {
      out[t * P + p] = v[0];
      continue;
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < K; ++j) {
      float f[8];
      unpack8(v[j], f);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        acc[i] = GATED ? fmaf(g[j], f[i], acc[i]) : acc[i] + f[i];
    }
    out[t * P + p] = pack8(acc);
  }
}

// out (M rows) [dest[t, j]] = g[t, j] * x (N rows) [t].  DG: also
// dgates[t, j] = x[t] . y (M rows) [dest[t, j]] in fp32.
template <int K, bool GATED, bool DG>
__global__ __launch_bounds__(ROW_BLOCK) void moe_scatter_kernel(
    const uint4* __restrict__ x, const int* __restrict__ dest,
    const float* __restrict__ gates, const uint4* __restrict__ y,
    uint4* __restrict__ out, float* __restrict__ dgates, long N, int P,
    long M) {
  const long t = (long)blockIdx.x * ROWS_PER_WG + threadIdx.x / WAVE;
  if (t >= N) return;
  const int lane = threadIdx.x & (WAVE - 1);
  long dst[K];
  float g[K], dot[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    dst[j] = row_piece0(dest, t * K + j, M, P);
    g[j] = GATED ? gates[t * K + j] : 1.f;
    dot[j] = 0.f;
  }
  for (int p = lane; p < P; p += WAVE) {
    const uint4 xv = x[t * P + p];
    if (!GATED) {
#pragma unroll
      for (int j = 0; j < K; ++j) out[dst[j] + p] = xv;
      continue;
    }
    uint4 yv[K];
    if (DG) {
#pragma unroll
      for (int j = 0; j < K; ++j) yv[j] = y[dst[j] + p];
    }
    float f[8];
    unpack8(xv, f);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      float r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = g[j] * f[i];
      out[dst[j] + p] = pack8(r);
      if (DG) {
        float q[8];
        unpack8(yv[j], q);
#pragma unroll
        for (int i = 0; i < 8; ++i) dot[j] = fmaf(f[i], q[i], dot[j]);
      }
    }
  }
  if (DG) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float s = wave_sum(dot[j]);
      if (lane == 0) dgates[t * K + j] = s;
    }
  }
}

struct RowArgs { long N, M; int K, P; };

RowArgs row_check(const torch::Tensor& rows_n, const torch::Tensor& rows_m,
                  const torch::Tensor& dest,
                  const c10::optional<torch::Tensor>& gates,
                  const char* what) {
  TORCH_CHECK(dest.is_cuda() && dest.scalar_type() == torch::kInt &&
              dest.dim() == 2 && dest.is_contiguous(), what,
              ": dest must be a contiguous (N, k) int32 CUDA tensor");
  const long N = dest.size(0), K = dest.size(1);
  TORCH_CHECK(K >= 1 && K <= MOE_ROUTE_MAX_K, what, ": k = ", K,
              " outside 1..", MOE_ROUTE_MAX_K);
  TORCH_CHECK(N * K < (1L << 31), what, ": N*k must stay below 2^31");
  for (const torch::Tensor* t : {&rows_n, &rows_m}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16 &&
                t->dim() == 2 && t->is_contiguous() &&
                t->size(1) % 8 == 0 && t->size(1) > 0 &&
                (uintptr_t)t->data_ptr() % 16 == 0, what,
                ": token buffers must be contiguous 16-byte aligned 2-D bf16 "
                "CUDA with D % 8 == 0");
  }
  TORCH_CHECK(rows_n.size(0) == N && rows_m.size(0) == N * K &&
              rows_n.size(1) == rows_m.size(1), what, ": expected (", N,
              ", D) and (", N * K, ", D) token buffers, got (",
              rows_n.size(0), ", ", rows_n.size(1), ") and (",
              rows_m.size(0), ", ", rows_m.size(1), ")");
  TORCH_CHECK(rows_n.size(1) / 8 < (1L << 31), what, ": D too large");
  if (gates.has_value())
    TORCH_CHECK(gates->is_cuda() && gates->scalar_type() == torch::kFloat &&
                gates->is_contiguous() && gates->dim() == 2 &&
                gates->size(0) == N && gates->size(1) == K, what,
                ": gates must be a contiguous (N, k) fp32 CUDA tensor");
  return RowArgs{N, N * K, (int)K, (int)(rows_n.size(1) / 8)};
}

unsigned row_grid(long N) {
  const long g = (N + ROWS_PER_WG - 1) / ROWS_PER_WG;
  TORCH_CHECK(g < (1L << 31), "moe_route: grid too large");
  return (unsigned)g;
}

#define MOE_K_SWITCH(k, ...)                                          \
  switch (k) {                                                        \
    case 1: { constexpr int K = 1; __VA_ARGS__; break; }              \
    case 2: { constexpr int K = 2; __VA_ARGS__; break; }              \
    case 3: { constexpr int K = 3; __VA_ARGS__; break; }              \
    case 4: { constexpr int K = 4; __VA_ARGS__; break; }              \
    case 5: { constexpr int K = 5; __VA_ARGS__; break; }              \
    case 6: { constexpr int K = 6; __VA_ARGS__; break; }              \
    case 7: { constexpr int K = 7; __VA_ARGS__; break; }              \
    default: { constexpr int K = 8; __VA_ARGS__; break; }             \
  }

}  // namespace

// (dest (N,k) int32, counts (E,) int64, offs (E+1,) int64)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> moe_route_plan(
    torch::Tensor topk_idx, int64_t num_experts) {
  TORCH_CHECK(topk_idx.is_cuda() && topk_idx.dim() == 2 &&
              topk_idx.is_contiguous() &&
              (topk_idx.scalar_type() == torch::kInt ||
               topk_idx.scalar_type() == torch::kLong),
              "moe_route_plan: topk_idx must be a contiguous (N, k) "
              "int32/int64 CUDA tensor");
  const long N = topk_idx.size(0), K = topk_idx.size(1), n = N * K;
  const int E = (int)num_experts;
  TORCH_CHECK(K >= 1 && K <= MOE_ROUTE_MAX_K, "moe_route_plan: k = ", K,
              " outside 1..", MOE_ROUTE_MAX_K);
  TORCH_CHECK(num_experts >= 1 && num_experts <= MOE_ROUTE_MAX_E,
              "moe_route_plan: num_experts = ", num_experts, " outside 1..",
              MOE_ROUTE_MAX_E);
  TORCH_CHECK(n < (1L << 31), "moe_route_plan: N*k must stay below 2^31");
  const auto iopt = topk_idx.options();
  auto dest = torch::empty({N, K}, iopt.dtype(torch::kInt));
  if (n == 0)
    return {dest, torch::zeros({E}, iopt.dtype(torch::kLong)),
            torch::zeros({E + 1}, iopt.dtype(torch::kLong))};
  auto counts = torch::empty({E}, iopt.dtype(torch::kLong));
  auto offs = torch::empty({E + 1}, iopt.dtype(torch::kLong));
  int nbits = 0;
  while ((1 << nbits) < E) ++nbits;
  const int ids64 = topk_idx.scalar_type() == torch::kLong ? 1 : 0;
  auto stream = at::cuda::getCurrentHIPStream();
  auto* cp = (long long*)counts.data_ptr();
  auto* op = (long long*)offs.data_ptr();
  if (n <= MOE_PLAN_CHUNK) {
    hipLaunchKernelGGL(moe_plan_small_kernel, dim3(1), dim3(PLAN_BLOCK), 0,
                       stream, topk_idx.data_ptr(), ids64, n, E, nbits, cp,
                       op, dest.data_ptr<int>());
    HIP_CHECK_LAST();
    return {dest, counts, offs};
  }
  const long nchunks = (n + MOE_PLAN_CHUNK - 1) / MOE_PLAN_CHUNK;
  auto block_hist = torch::empty({nchunks, E}, iopt.dtype(torch::kInt));
  hipLaunchKernelGGL(moe_plan_hist_kernel, dim3((unsigned)nchunks),
                     dim3(PLAN_BLOCK), 0, stream, topk_idx.data_ptr(), ids64,
                     n, E, block_hist.data_ptr<int>());
  hipLaunchKernelGGL(moe_plan_scan_kernel, dim3(1), dim3(PLAN_BLOCK), 0,
                     stream, block_hist.data_ptr<int>(), (int)nchunks, E, cp,
                     op);
  hipLaunchKernelGGL(moe_plan_rank_kernel, dim3((unsigned)nchunks),
                     dim3(PLAN_BLOCK), 0, stream, topk_idx.data_ptr(), ids64,
                     n, E, nbits, block_hist.data_ptr<int>(), op,
                     dest.data_ptr<int>());
  HIP_CHECK_LAST();
  return {dest, counts, offs};
}

// out (N, D) = sum_j gates[t, j] * y[dest[t, j]]; gates None = unit gates
torch::Tensor moe_route_gather(torch::Tensor y, torch::Tensor dest,
                               c10::optional<torch::Tensor> gates) {
  TORCH_CHECK(y.dim() == 2 && dest.dim() == 2,
              "moe_route_gather: y and dest must be 2-D");
  auto out = torch::empty({dest.size(0), y.size(1)}, y.options());
  const RowArgs a = row_check(out, y, dest, gates, "moe_route_gather");
  if (a.N == 0) return out;
  auto stream = at::cuda::getCurrentHIPStream();
  const auto* yp = (const uint4*)y.data_ptr();
  auto* outp = (uint4*)out.data_ptr();
  const int* dp = dest.data_ptr<int>();
  if (gates.has_value()) {
    const float* gp = gates->data_ptr<float>();
    MOE_K_SWITCH(a.K, hipLaunchKernelGGL(
        (moe_gather_kernel<K, true>), dim3(row_grid(a.N)), dim3(ROW_BLOCK),
        0, stream, yp, dp, gp, outp, a.N, a.P, a.M));
  } else {
    MOE_K_SWITCH(a.K, hipLaunchKernelGGL(
        (moe_gather_kernel<K, false>), dim3(row_grid(a.N)), dim3(ROW_BLOCK),
        0, stream, yp, dp, (const float*)nullptr, outp, a.N, a.P, a.M));
  }
  HIP_CHECK_LAST();
  return out;
}

// out (N*k, D)[dest[t, j]] = gates[t, j] * x[t]; with y (N*k, D) also
// dgates (N, k) fp32 = x[t] . y[dest[t, j]].  y needs gates.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> moe_route_scatter(
    torch::Tensor x, torch::Tensor dest, c10::optional<torch::Tensor> gates,
    c10::optional<torch::Tensor> y) {
  TORCH_CHECK(!y.has_value() || gates.has_value(),
              "moe_route_scatter: dgates needs gates");
  TORCH_CHECK(x.dim() == 2 && dest.dim() == 2,
              "moe_route_scatter: x and dest must be 2-D");
  auto out = torch::empty({dest.numel(), x.size(1)}, x.options());
  c10::optional<torch::Tensor> dg;
  if (y.has_value())
    dg = torch::empty({dest.size(0), dest.size(1)},
                      x.options().dtype(torch::kFloat));
  const RowArgs a = row_check(x, out, dest, gates, "moe_route_scatter");
  if (y.has_value()) row_check(x, *y, dest, gates, "moe_route_scatter");
  if (a.N == 0) return {out, dg};
  auto stream = at::cuda::getCurrentHIPStream();
  const auto* xp = (const uint4*)x.data_ptr();
  auto* outp = (uint4*)out.data_ptr();
  const int* dp = dest.data_ptr<int>();
  if (!gates.has_value()) {
    MOE_K_SWITCH(a.K, hipLaunchKernelGGL(
        (moe_scatter_kernel<K, false, false>), dim3(row_grid(a.N)),
        dim3(ROW_BLOCK), 0, stream, xp, dp, (const float*)nullptr,
        (const uint4*)nullptr, outp, (float*)nullptr, a.N, a.P, a.M));
  } else if (!y.has_value()) {
    const float* gp = gates->data_ptr<float>();
    MOE_K_SWITCH(a.K, hipLaunchKernelGGL(
        (moe_scatter_kernel<K, true, false>), dim3(row_grid(a.N)),
        dim3(ROW_BLOCK), 0, stream, xp, dp, gp, (const uint4*)nullptr, outp,
        (float*)nullptr, a.N, a.P, a.M));
  } else {
    const float* gp = gates->data_ptr<float>();
    MOE_K_SWITCH(a.K, hipLaunchKernelGGL(
        (moe_scatter_kernel<K, true, true>), dim3(row_grid(a.N)),
        dim3(ROW_BLOCK), 0, stream, xp, dp, gp, (const uint4*)y->data_ptr(),
        outp, dg->data_ptr<float>(), a.N, a.P, a.M));
  }
  HIP_CHECK_LAST();
  return {out, dg};
}
