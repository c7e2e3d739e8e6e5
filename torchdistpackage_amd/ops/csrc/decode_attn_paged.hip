// Paged bf16 KV cache: split-KV decode attention through a block table, and
// the append that writes through it.
//
// A paged cache (K or V) is a pool (P, Hkv, page, D) bf16 plus a block table
// (B, NB) int32 shared by K and V: entry [b, i] is the pool page that holds
// positions [i*page, (i+1)*page) of sequence b; page is a power of two in
// 16..128 and the capacity is Smax = NB*page.
//
// Attention.  The contract, the work split, the lane-to-key mapping and the
// order of every sum and merge are decode_attn.hip's: the kernel body is the
// same text (decode_attn_body.inc), so on the same values at the same chunk
// length the result is bit-equal to the contiguous kernel's.  What the table
// adds:
//  - a workgroup's chunk is a whole number of pages (da_choose_chunk_paged:
//    a multiple of max(64, page), from capacity and CU count only, so a
//    captured grid stays valid while sequences grow and the host rewrites
//    the table's contents)
//  - at entry the workgroup reads the page ids of the part of its chunk
//    below the valid length with one coalesced load, clamps each to
//    [0, P-1], stores them to LDS and takes one barrier.  The LDS array is
//    dynamic, chunk/page ints (at most DA_MAX_IDS = 4096, 16 KB; a chunk
//    that would need more is shortened and nsplit grows), so a short chunk
//    does not pay occupancy for a long one's table
//  - the key loop forms an address as
//      pool + ((id*Hkv + h)*page + (j & (page-1)))*D + ld*8
//    with id read from LDS at (j - c0) >> log2(page); j is already clamped
//    into [c0, c1-1].  The D/8 lanes of a key read one LDS word (broadcast)
//    and no global load sits in front of a K/V load
//  - table entries at or past the valid length are never read; a stale entry
//    that is read may give a wrong answer, never an out-of-range access
//  - partials and the second launch are the contiguous kernel's (da_combine)
//
// Append (one launch for K and V): D/8 lanes own one destination row and
// move 16 bytes each; the page id (clamped) and the in-page offset are
// computed per row.  The position is a kernel argument or is read from an
// int64 device tensor (1 or B elements), clamped to [0, Smax-S] before any
// address is formed, so the launch captures into a hipGraph.
//
// The file is built without packed-fp32 VALU forms (ops/build.py gives it the
// compiler flag, as a translation unit of the _tdpa_nopk module), like the
// fp8 cache kernels.  A flag and not a function attribute: a callee whose
// target features differ from its caller's is never inlined, and under an
// attribute every __shfl_xor, __syncthreads and make_uint4 of the body became
// an out-of-line call.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "decode_attn_common.h"

#define KVP_BLOCK 256

DEVINL int dap_page_id(const int* __restrict__ p, int P) {
  return min(max(*p, 0), P - 1);
}

template <int D, int MT>
__global__ __launch_bounds__(DA_BLOCK) void decode_attn_paged_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kpool,
    const ushort* __restrict__ vpool, const int* __restrict__ table,
    ushort* __restrict__ out, float* __restrict__ part_acc,
    float* __restrict__ part_ml, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int P, int NB, int lg_page, long q_sb, long q_sh,
    long q_ss, long o_sb, long o_sh, long o_ss, float scale_log2) {
  extern __shared__ int sm_ids[];     // clamped page ids of [c0, c1)
  // c0 is a multiple of the chunk, the chunk of the page: the first page of
  // the chunk is c0 >> lg_page, and c1 <= Smax keeps every index below NB
#define DA_SRC_INIT()                                                        \
  const int pmask = (1 << lg_page) - 1;                                      \
  {                                                                          \
    const int* row = table + (long)b * NB + (c0 >> lg_page);                 \
    const int nid = (c1 - c0 + pmask) >> lg_page;                            \
    for (int i = threadIdx.x; i < nid; i += DA_BLOCK)                        \
      sm_ids[i] = dap_page_id(row + i, P);                                   \
  }                                                                          \
  __syncthreads();                                                           \
  const long pg_stride = ((long)Hkv << lg_page) * D; /* elements per page */ \
  const long hoff = ((long)h << lg_page) * D + ld * 8;                       \
  const ushort* kbase = kpool + hoff;                                        \
  const ushort* vbase = vpool + hoff
#define DAP_OFF(j)                                        \
  ((long)sm_ids[((j) - c0) >> lg_page] * pg_stride +      \
   (long)(((j) & pmask) * D))
#define DA_KPTR(j) (&kbase[DAP_OFF(j)])
#define DA_VPTR(j) (&vbase[DAP_OFF(j)])
#include "decode_attn_body.inc"
#undef DA_SRC_INIT
#undef DAP_OFF
#undef DA_KPTR
#undef DA_VPTR
}

template <int D>
__global__ __launch_bounds__(D) void decode_attn_paged_combine_kernel(
    const float* __restrict__ part_acc, const float* __restrict__ part_ml,
    ushort* __restrict__ out, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int Hkv, int G, int Sq, int Smax,
    int chunk, int nsplit, int MT, long o_sb, long o_sh, long o_ss) {
  da_combine<D>(part_acc, part_ml, out, pos_ptr, pos_stride, pos_host, Hkv, G,
                Sq, Smax, chunk, nsplit, MT, o_sb, o_sh, o_ss);
}

// rows are numbered (kv, b, h, s): kv = 0 takes k into the K pool, 1 takes
// v into the V pool
template <int D>
__global__ __launch_bounds__(KVP_BLOCK) void kv_paged_append_kernel(
    const ushort* __restrict__ k, const ushort* __restrict__ v,
    ushort* __restrict__ kpool, ushort* __restrict__ vpool,
    const int* __restrict__ table, const long* __restrict__ pos_ptr,
    int pos_stride, long pos_host, int B, int Hkv, int S, int Smax, int P,
    int NB, int lg_page, long k_sb, long k_sh, long k_ss, long v_sb,
    long v_sh, long v_ss) {
  constexpr int LPR = D / 8;                 // lanes per row
  constexpr int RPB = KVP_BLOCK / LPR;       // rows per block
  const long nrow = (long)B * Hkv * S;       // per tensor
  const long r = (long)blockIdx.x * RPB + threadIdx.x / LPR;
  if (r >= 2 * nrow) return;
  const int ld = threadIdx.x % LPR;
  const bool is_v = r >= nrow;
  const long rr = is_v ? r - nrow : r;
  const int s = (int)(rr % S);
  const int h = (int)((rr / S) % Hkv);
  const int b = (int)(rr / ((long)S * Hkv));
  // p0 <= Smax - S, so pos < Smax = NB << lg_page and pos >> lg_page < NB
  const int pos = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, S) + s;
  const int id = dap_page_id(table + (long)b * NB + (pos >> lg_page), P);
  const long drow = (((long)id * Hkv + h) << lg_page) +
                    (pos & ((1 << lg_page) - 1));
  const ushort* src = is_v ? v + (long)b * v_sb + (long)h * v_sh + (long)s * v_ss
                           : k + (long)b * k_sb + (long)h * k_sh + (long)s * k_ss;
  ushort* dst = is_v ? vpool : kpool;
  *(uint4*)&dst[drow * D + ld * 8] = *(const uint4*)&src[ld * 8];
}

// pools (P, Hkv, page, D) and the table (B, NB); returns log2(page)
static int dap_check_cache(const torch::Tensor& kpool,
                           const torch::Tensor& vpool,
                           const torch::Tensor& table, int B, int Hkv, int D,
                           const char* op) {
  for (const torch::Tensor* t : {&kpool, &vpool})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16 &&
                    t->dim() == 4 && t->is_contiguous() &&
                    ((uintptr_t)t->data_ptr()) % 16 == 0,
                op, ": a paged pool must be contiguous 4-D bf16 CUDA, "
                "16-byte aligned");
  TORCH_CHECK(vpool.sizes() == kpool.sizes() && kpool.size(1) == Hkv &&
                  kpool.size(3) == D,
              op, ": pool shape mismatch");
  const long page = kpool.size(2);
  TORCH_CHECK(page >= 16 && page <= 128 && (page & (page - 1)) == 0, op,
              ": page size must be a power of two in 16..128, got ", page);
  TORCH_CHECK(kpool.size(0) >= 1 && kpool.size(0) < (1L << 31), op,
              ": pool page count out of range");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt &&
                  table.dim() == 2 && table.is_contiguous() &&
                  table.size(0) == B && table.size(1) >= 1 &&
                  table.get_device() == kpool.get_device(),
              op, ": block_table must be contiguous int32 (B, NB) on the "
              "pool's device");
  TORCH_CHECK(table.size(1) * page < (1L << 30), op, ": capacity too large");
  int lg = 0;
  while ((1L << lg) < page) ++lg;
  return lg;
}

static void dap_check_rows(const torch::Tensor& t, const char* op,
                           const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 4 && t.stride(3) == 1,
              op, ": ", name,
              " must be 4-D bf16 CUDA with contiguous head dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr()) % 16 == 0,
              op, ": ", name,
              " must allow 16-byte loads (strides % 8, 16-byte base)");
}

static const long* dap_pos(const c10::optional<torch::Tensor>& pos_t,
                           long pos0, int B, long rows, long Smax,
                           const char* op, int* pos_stride) {
  *pos_stride = 0;
  if (pos_t.has_value()) {
    TORCH_CHECK(pos_t->is_cuda() && pos_t->scalar_type() == torch::kLong &&
                    pos_t->is_contiguous() &&
                    (pos_t->numel() == 1 || pos_t->numel() == B),
                op, ": pos0 tensor must be int64 CUDA with 1 or B elements");
    *pos_stride = pos_t->numel() == 1 ? 0 : 1;
    return (const long*)pos_t->data_ptr();
  }
  TORCH_CHECK(pos0 >= 0 && pos0 + rows <= Smax, op, ": pos0=", pos0, " with ",
              rows, " rows outside the cache (Smax=", Smax, ")");
  return nullptr;
}

// Same arguments as decode_attention, with each cache as its pool and the
// shared block table.
torch::Tensor decode_attention_paged(torch::Tensor q, torch::Tensor k_pool,
                                     torch::Tensor v_pool,
                                     torch::Tensor block_table,
                                     torch::Tensor out,
                                     c10::optional<torch::Tensor> pos_t,
                                     long pos0, double scale, long split_kv) {
  const char* op = "decode_attention";
  dap_check_rows(q, op, "q");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 &&
              out.dim() == 4 && out.stride(3) == 1);
  const int B = q.size(0), Hq = q.size(1), Sq = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128,
              "decode_attention: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(k_pool.dim() == 4, "decode_attention: pool must be 4-D");
  const int Hkv = k_pool.size(1);
  const int lg_page = dap_check_cache(k_pool, v_pool, block_table, B, Hkv, D,
                                      op);
  const int page = 1 << lg_page;
  const int P = k_pool.size(0), NB = block_table.size(1);
  const int Smax = NB * page;
  TORCH_CHECK(out.size(0) == B && out.size(1) == Hq && out.size(2) == Sq &&
              out.size(3) == D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "decode_attention: Hq % Hkv != 0");
  TORCH_CHECK(Sq >= 1 && Smax >= Sq);
  const int G = Hq / Hkv;
  const int M = G * Sq;
  TORCH_CHECK(M <= DA_MAX_M, "decode_attention: (Hq/Hkv)*Sq = ", M,
              " exceeds the kernel's ", DA_MAX_M, " query rows per kv head");
  int pos_stride;
  const long* pos_ptr = dap_pos(pos_t, pos0, B, Sq, Smax, op, &pos_stride);
  TORCH_CHECK(split_kv >= 0);

  // split choice from the capacity only, so a captured grid stays valid
  const int BH = B * Hkv;
  const int chunk = da_choose_chunk_paged(
      Smax, BH, split_kv,
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount, page);
  const int nsplit = (Smax + chunk - 1) / chunk;
  TORCH_CHECK(nsplit <= 65535);
  const size_t ids_bytes = (size_t)(chunk >> lg_page) * sizeof(int);

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
  const ushort* kp = (const ushort*)k_pool.data_ptr();
  const ushort* vp = (const ushort*)v_pool.data_ptr();
  const int* tp = block_table.data_ptr<int>();
  ushort* optr = (ushort*)out.data_ptr();
#define DAP_LAUNCH(D_, MT_)                                                  \
  hipLaunchKernelGGL((decode_attn_paged_kernel<D_, MT_>), grid, block,       \
                     ids_bytes, stream, qp, kp, vp, tp, optr, pa, pm,        \
                     pos_ptr, pos_stride, pos0, Hkv, G, Sq, Smax, chunk,     \
                     nsplit, P, NB, lg_page, q.stride(0), q.stride(1),       \
                     q.stride(2), out.stride(0), out.stride(1),              \
                     out.stride(2), scale_log2)
#define DAP_DISPATCH(D_)                \
  switch (MT) {                         \
    case 1: DAP_LAUNCH(D_, 1); break;   \
    case 2: DAP_LAUNCH(D_, 2); break;   \
    case 4: DAP_LAUNCH(D_, 4); break;   \
    case 8: DAP_LAUNCH(D_, 8); break;   \
    default: DAP_LAUNCH(D_, 16); break; \
  }
  if (D == 64) { DAP_DISPATCH(64) } else { DAP_DISPATCH(128) }
#undef DAP_DISPATCH
#undef DAP_LAUNCH
  HIP_CHECK_LAST();
  if (nsplit > 1) {
    const dim3 cgrid((unsigned)BH, (unsigned)M);
#define DAP_COMBINE(D_)                                                      \
  hipLaunchKernelGGL((decode_attn_paged_combine_kernel<D_>), cgrid,          \
                     dim3(D_), 0, stream, pa, pm, optr, pos_ptr, pos_stride, \
                     pos0, Hkv, G, Sq, Smax, chunk, nsplit, MT,              \
                     out.stride(0), out.stride(1), out.stride(2))
    if (D == 64) DAP_COMBINE(64); else DAP_COMBINE(128);
#undef DAP_COMBINE
    HIP_CHECK_LAST();
  }
  return out;
}

// k, v (B, Hkv, S, D) bf16 -> positions [pos, pos+S) of both paged caches,
// one launch.  pos_t: optional int64 device tensor (1 or B elements) that
// overrides pos0.
void kv_paged_append(torch::Tensor k_pool, torch::Tensor v_pool,
                     torch::Tensor block_table, torch::Tensor k,
                     torch::Tensor v, c10::optional<torch::Tensor> pos_t,
                     long pos0) {
  const char* op = "kv_cache_append";
  dap_check_rows(k, op, "k");
  dap_check_rows(v, op, "v");
  const int B = k.size(0), Hkv = k.size(1), D = k.size(3);
  const long S = k.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "kv_cache_append: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(v.sizes() == k.sizes(), "kv_cache_append: k/v shape mismatch");
  const int lg_page = dap_check_cache(k_pool, v_pool, block_table, B, Hkv, D,
                                      op);
  const int P = k_pool.size(0), NB = block_table.size(1);
  const long Smax = (long)NB << lg_page;
  TORCH_CHECK(S >= 1 && S <= Smax);
  int pos_stride;
  const long* pos_ptr = dap_pos(pos_t, pos0, B, S, Smax, op, &pos_stride);
  const long rows = 2L * B * Hkv * S;
  const int rpb = KVP_BLOCK / (D / 8);
  const long nblk = (rows + rpb - 1) / rpb;
  TORCH_CHECK(nblk < (1L << 31));
  auto stream = at::cuda::getCurrentHIPStream();
#define KVP_APPEND(D_)                                                       \
  hipLaunchKernelGGL((kv_paged_append_kernel<D_>), dim3((unsigned)nblk),     \
                     dim3(KVP_BLOCK), 0, stream,                             \
                     (const ushort*)k.data_ptr(), (const ushort*)v.data_ptr(), \
                     (ushort*)k_pool.data_ptr(), (ushort*)v_pool.data_ptr(), \
                     block_table.data_ptr<int>(), pos_ptr, pos_stride, pos0, \
                     B, Hkv, (int)S, (int)Smax, P, NB, lg_page, k.stride(0), \
                     k.stride(1), k.stride(2), v.stride(0), v.stride(1),     \
                     v.stride(2))
  if (D == 64) KVP_APPEND(64); else KVP_APPEND(128);
#undef KVP_APPEND
  HIP_CHECK_LAST();
}
