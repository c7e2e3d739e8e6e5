// RMSNorm + LayerNorm forward/backward for gfx950.
//
// Memory-bound ops: one 256-thread workgroup per row (grid-strided over
// rows), bf16 traffic vectorized 8-wide (ushort4 pairs = 16 B/lane), f32
// accumulation, rstd/mean saved for backward.  dweight/dbias are accumulated
// in LDS per block, then atomically added to fp32 global buffers (one atomic
// per column per block).
//
// Replaces the reference's nn.LayerNorm hot path
// (/root/reference/torchdistpackage/parallel/tensor_parallel/transformer.py:15-44)
// and the layernorm math spec (explore/understand_ops/layernorm.py:3-14).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "fused_checks.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_D = 16384;

// ---------------------------------------------------------------- RMSNorm

template <typename T>
DEVINL float load_as_f32(const T* p, int i);
template <> DEVINL float load_as_f32<bf16_t>(const bf16_t* p, int i) {
  return bf2f(((const unsigned short*)p)[i]);
}
template <> DEVINL float load_as_f32<float>(const float* p, int i) {
  return p[i];
}
template <typename T>
DEVINL void store_from_f32(T* p, int i, float v);
template <> DEVINL void store_from_f32<bf16_t>(bf16_t* p, int i, float v) {
  ((unsigned short*)p)[i] = f2bf(v);
}
template <> DEVINL void store_from_f32<float>(float* p, int i, float v) {
  p[i] = v;
}

template <typename T>
__global__ void rmsnorm_fwd_kernel(const T* __restrict__ x,
                                   const T* __restrict__ w,
                                   T* __restrict__ y,
                                   float* __restrict__ rstd,
                                   int rows, int D, float eps) {
  __shared__ float lds[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + (long)row * D;
    T* yr = y + (long)row * D;
    float ss = 0.f;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float v = load_as_f32(xr, i);
      ss += v * v;
    }
    ss = block_sum<BLOCK>(ss, lds);
    float r = rsqrtf(ss / D + eps);
    if (threadIdx.x == 0) rstd[row] = r;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float v = load_as_f32(xr, i);
      float wv = load_as_f32(w, i);
      store_from_f32(yr, i, v * r * wv);
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void rmsnorm_bwd_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x,
                                   const T* __restrict__ w,
                                   const float* __restrict__ rstd,
                                   T* __restrict__ dx,
                                   int rows, int D) {
  // dx only: dw comes from norm_bwd_dwdb_kernel
  __shared__ float scratch[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + (long)row * D;
    const T* xr = x + (long)row * D;
    T* dxr = dx + (long)row * D;
    float r = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float xhat = load_as_f32(xr, i) * r;
      float wdy = load_as_f32(w, i) * load_as_f32(dyr, i);
      dot += wdy * xhat;
    }
    dot = block_sum<BLOCK>(dot, scratch) / D;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float xhat = load_as_f32(xr, i) * r;
      float dyv = load_as_f32(dyr, i);
      float wdy = load_as_f32(w, i) * dyv;
      store_from_f32(dxr, i, r * (wdy - xhat * dot));
    }
    __syncthreads();
  }
}

// dw (and db) of the norm backwards outside the bf16 register path, in a
// fixed order.  Those kernels used to add every block's dw into one fp32
// row with atomicAdd, gridDim deep, so dw depended on the order the blocks
// arrived in (measured on 2050 x 64 fp32: 2.8e-7 to 1.08e-5 relative from
// run to run) and needed [D] (LayerNorm: [2D]) floats of dynamic LDS.  Here
// a block owns DW_COLS columns; its DW_LANES row lanes each sum every
// DW_LANES-th row in row order, and lane 0 adds the lane sums in lane
// order.  MEAN == false is RMSNorm (xhat = x * rstd, no db).
constexpr int DW_COLS = 16;
constexpr int DW_LANES = BLOCK / DW_COLS;

template <typename T, bool MEAN>
__global__ void norm_bwd_dwdb_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ dw,
                                     float* __restrict__ db,
                                     int rows, int D) {
  __shared__ float lds_w[DW_LANES][DW_COLS];
  __shared__ float lds_b[DW_LANES][DW_COLS];
  const int c = threadIdx.x % DW_COLS;
  const int lane = threadIdx.x / DW_COLS;
  const int col = blockIdx.x * DW_COLS + c;
  float aw = 0.f, ab = 0.f;
  if (col < D) {
    for (int row = lane; row < rows; row += DW_LANES) {
      const long off = (long)row * D;
      float xv = load_as_f32(x + off, col);
      float dyv = load_as_f32(dy + off, col);
      float xhat = MEAN ? (xv - mean[row]) * rstd[row] : xv * rstd[row];
      aw += dyv * xhat;
      ab += dyv;
    }
  }
  lds_w[lane][c] = aw;
  lds_b[lane][c] = ab;
  __syncthreads();
  if (lane == 0 && col < D) {
    float sw = 0.f, sb = 0.f;
    for (int l = 0; l < DW_LANES; ++l) {
      sw += lds_w[l][c];
      sb += lds_b[l][c];
    }
    dw[col] = sw;
    if (MEAN) db[col] = sb;
  }
}

// -------------------------------------------------------------- LayerNorm

// LayerNorm statistics.  The one-pass form var = ss/D - mu^2 has a relative
// error of about (1 + mu^2/var) ulps: fine on centred rows, catastrophic once
// |mean| >> std (measured: a 1000 + randn fp32 row got an rstd 11% off, a
// 100 + 1e-3*randn row a negative variance and NaN).  So the one-pass
// result is kept only while mu^2 <= var, where it is as good as any; every
// other row (NaN included) takes a second pass: the sums of (x - mu0) and
// (x - mu0)^2, the first of which also refines the mean.  The test is
// uniform over the block.
DEVINL bool ln_one_pass_ok(float mu, float var) { return mu * mu <= var; }

DEVINL void ln_finish_stats(float mu0, float d1, float d2, int D, float eps,
                            float& mu, float& r) {
  const float c = d1 / D;
  mu = mu0 + c;
  const float var = fmaxf(d2 / D - c * c, 0.f);
  r = rsqrtf(var + eps);
}

template <typename T>
__global__ void layernorm_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ w,
                                     const T* __restrict__ b,
                                     T* __restrict__ y,
                                     float* __restrict__ mean,
                                     float* __restrict__ rstd,
                                     int rows, int D, float eps) {
  __shared__ float lds[3 * BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + (long)row * D;
    T* yr = y + (long)row * D;
    float s = 0.f, ss = 0.f;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float v = load_as_f32(xr, i);
      s += v;
      ss += v * v;
    }
    s = block_sum<BLOCK>(s, lds);
    __syncthreads();
    ss = block_sum<BLOCK>(ss, lds);
    float mu = s / D;
    float var = ss / D - mu * mu;
    float r = rsqrtf(var + eps);
    if (!ln_one_pass_ok(mu, var)) {
      const float mu0 = mu;
      float d1 = 0.f, d2 = 0.f;
      for (int i = threadIdx.x; i < D; i += BLOCK) {
        float d = load_as_f32(xr, i) - mu0;
        d1 += d;
        d2 += d * d;
      }
      d1 = block_sum<BLOCK>(d1, lds + BLOCK / WAVE);
      d2 = block_sum<BLOCK>(d2, lds + 2 * BLOCK / WAVE);
      ln_finish_stats(mu0, d1, d2, D, eps, mu, r);
    }
    if (threadIdx.x == 0) { mean[row] = mu; rstd[row] = r; }
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float v = load_as_f32(xr, i);
      float wv = load_as_f32(w, i);
      float bv = load_as_f32(b, i);
      store_from_f32(yr, i, (v - mu) * r * wv + bv);
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void layernorm_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const T* __restrict__ w,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     T* __restrict__ dx,
                                     int rows, int D) {
  // dx only: dw and db come from norm_bwd_dwdb_kernel
  __shared__ float scratch[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + (long)row * D;
    const T* xr = x + (long)row * D;
    T* dxr = dx + (long)row * D;
    float mu = mean[row], r = rstd[row];
    float m1 = 0.f, m2 = 0.f;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float xhat = (load_as_f32(xr, i) - mu) * r;
      float wdy = load_as_f32(w, i) * load_as_f32(dyr, i);
      m1 += wdy;
      m2 += wdy * xhat;
    }
    m1 = block_sum<BLOCK>(m1, scratch);
    __syncthreads();
    m2 = block_sum<BLOCK>(m2, scratch);
    m1 /= D;
    m2 /= D;
    for (int i = threadIdx.x; i < D; i += BLOCK) {
      float xhat = (load_as_f32(xr, i) - mu) * r;
      float dyv = load_as_f32(dyr, i);
      float wdy = load_as_f32(w, i) * dyv;
      store_from_f32(dxr, i, r * (wdy - m1 - xhat * m2));
    }
    __syncthreads();
  }
}

int pick_grid(long rows) {
  // memory-bound: cap at 2048 blocks, grid-stride the rest (guideline 11)
  long g = rows < 2048 ? rows : 2048;
  return (int)(g > 0 ? g : 1);
}

// ------------------- vectorized bf16 variants (D % 8 == 0) ----------------
// 16 B/lane loads (guideline 13: scalar bf16 is 2-2.5x slower).

typedef ushort4 u4;
struct f8 { float v[8]; };

DEVINL f8 load8f(const unsigned short* p) {
  u4 a = *(const u4*)p;
  u4 b = *(const u4*)(p + 4);
  f8 r;
  r.v[0] = bf2f(a.x); r.v[1] = bf2f(a.y); r.v[2] = bf2f(a.z); r.v[3] = bf2f(a.w);
  r.v[4] = bf2f(b.x); r.v[5] = bf2f(b.y); r.v[6] = bf2f(b.z); r.v[7] = bf2f(b.w);
  return r;
}

DEVINL void store8f(unsigned short* p, const f8& r) {
  u4 a, b;
  a.x = f2bf(r.v[0]); a.y = f2bf(r.v[1]); a.z = f2bf(r.v[2]); a.w = f2bf(r.v[3]);
  b.x = f2bf(r.v[4]); b.y = f2bf(r.v[5]); b.z = f2bf(r.v[6]); b.w = f2bf(r.v[7]);
  *(u4*)p = a;
  *(u4*)(p + 4) = b;
}

__global__ void rmsnorm_fwd_bf16v8(const unsigned short* __restrict__ x,
                                   const unsigned short* __restrict__ w,
                                   unsigned short* __restrict__ y,
                                   float* __restrict__ rstd,
                                   int rows, int D, float eps) {
  __shared__ float lds[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* xr = x + (long)row * D;
    unsigned short* yr = y + (long)row * D;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 v = load8f(xr + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v.v[j] * v.v[j];
    }
    ss = block_sum<BLOCK>(ss, lds);
    float r = rsqrtf(ss / D + eps);
    if (threadIdx.x == 0) rstd[row] = r;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 v = load8f(xr + i);
      f8 wv = load8f(w + i);
      f8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) out.v[j] = v.v[j] * r * wv.v[j];
      store8f(yr + i, out);
    }
    __syncthreads();
  }
}

__global__ void rmsnorm_bwd_bf16v8(const unsigned short* __restrict__ dy,
                                   const unsigned short* __restrict__ x,
                                   const unsigned short* __restrict__ w,
                                   const float* __restrict__ rstd,
                                   unsigned short* __restrict__ dx,
                                   int rows, int D) {
  // dx only: dw comes from norm_bwd_dwdb_kernel
  __shared__ float scratch[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + (long)row * D;
    const unsigned short* xr = x + (long)row * D;
    unsigned short* dxr = dx + (long)row * D;
    float r = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 xv = load8f(xr + i), dyv = load8f(dyr + i), wv = load8f(w + i);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dot += wv.v[j] * dyv.v[j] * xv.v[j] * r;
    }
    dot = block_sum<BLOCK>(dot, scratch) / D;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 xv = load8f(xr + i), dyv = load8f(dyr + i), wv = load8f(w + i);
      f8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = xv.v[j] * r;
        out.v[j] = r * (wv.v[j] * dyv.v[j] - xhat * dot);
      }
      store8f(dxr + i, out);
    }
    __syncthreads();
  }
}

// The row's chunks stay in registers (NC chunks of 8 per thread, as in the
// *_reg backward kernels): x is read from memory once, and the second pass
// of an off-centre row costs no memory traffic.
//
// RES == true is the fused junction: the row normalised is
// x_new = bf16(x + bf16(lin + lbias)), formed in registers from the linear
// output ``lin``, its bias (may be null) and the residual stream x, and
// stored to ``xnew``.  The two bf16 roundings are those of the unfused
// ``x + (lin + lbias)``, and everything after them is the RES == false code
// on the same values in the same order, so x_new, y, mean and rstd are
// bit-identical to layer_norm(x + (lin + lbias)).
template <int NC, bool RES>
__global__ void __launch_bounds__(BLOCK)
layernorm_fwd_bf16v8(const unsigned short* __restrict__ x,
                     const unsigned short* __restrict__ lin,
                     const unsigned short* __restrict__ lbias,
                     const unsigned short* __restrict__ w,
                     const unsigned short* __restrict__ b,
                     unsigned short* __restrict__ xnew,
                     unsigned short* __restrict__ y,
                     float* __restrict__ mean,
                     float* __restrict__ rstd,
                     int rows, int D, float eps) {
  __shared__ float lds[4 * BLOCK / WAVE];
  const int wid = threadIdx.x / WAVE;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* xr = x + (long)row * D;
    unsigned short* yr = y + (long)row * D;
    f8 xv[NC];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        xv[c] = load8f(xr + i);
        if constexpr (RES) {
          f8 t = load8f(lin + (long)row * D + i);
          if (lbias != nullptr) {
            f8 lb = load8f(lbias + i);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              t.v[j] = bf2f(f2bf(t.v[j] + lb.v[j]));
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
            xv[c].v[j] = bf2f(f2bf(xv[c].v[j] + t.v[j]));
          store8f(xnew + (long)row * D + i, xv[c]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s += xv[c].v[j];
          ss += xv[c].v[j] * xv[c].v[j];
        }
      }
    }
    // two block sums behind one barrier: separate scratch quarters
    {
      float sw = wave_sum(s), ssw = wave_sum(ss);
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        lds[wid] = sw;
        lds[BLOCK / WAVE + wid] = ssw;
      }
      __syncthreads();
      s = 0.f; ss = 0.f;
#pragma unroll
      for (int i = 0; i < BLOCK / WAVE; ++i) {
        s += lds[i];
        ss += lds[BLOCK / WAVE + i];
      }
    }
    float mu = s / D;
    float var = ss / D - mu * mu;
    float r = rsqrtf(var + eps);
    if (!ln_one_pass_ok(mu, var)) {
      const float mu0 = mu;
      float d1 = 0.f, d2 = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        int i = threadIdx.x * 8 + c * BLOCK * 8;
        if (i < D) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float d = xv[c].v[j] - mu0;
            d1 += d;
            d2 += d * d;
          }
        }
      }
      float a = wave_sum(d1), q = wave_sum(d2);
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        lds[2 * BLOCK / WAVE + wid] = a;
        lds[3 * BLOCK / WAVE + wid] = q;
      }
      __syncthreads();
      d1 = 0.f; d2 = 0.f;
#pragma unroll
      for (int i = 0; i < BLOCK / WAVE; ++i) {
        d1 += lds[2 * BLOCK / WAVE + i];
        d2 += lds[3 * BLOCK / WAVE + i];
      }
      ln_finish_stats(mu0, d1, d2, D, eps, mu, r);
    }
    if (threadIdx.x == 0) { mean[row] = mu; rstd[row] = r; }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        f8 wv = load8f(w + i), bv = load8f(b + i);
        f8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          out.v[j] = (xv[c].v[j] - mu) * r * wv.v[j] + bv.v[j];
        store8f(yr + i, out);
      }
    }
    __syncthreads();
  }
}

__global__ void layernorm_bwd_bf16v8(const unsigned short* __restrict__ dy,
                                     const unsigned short* __restrict__ x,
                                     const unsigned short* __restrict__ w,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     unsigned short* __restrict__ dx,
                                     int rows, int D) {
  // dx only: dw and db come from norm_bwd_dwdb_kernel
  __shared__ float scratch[2 * BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + (long)row * D;
    const unsigned short* xr = x + (long)row * D;
    unsigned short* dxr = dx + (long)row * D;
    float mu = mean[row], r = rstd[row];
    float m1 = 0.f, m2 = 0.f;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 xv = load8f(xr + i), dyv = load8f(dyr + i), wv = load8f(w + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = (xv.v[j] - mu) * r;
        float wdy = wv.v[j] * dyv.v[j];
        m1 += wdy;
        m2 += wdy * xhat;
      }
    }
    {
      const int wid = threadIdx.x / WAVE;
      float a = wave_sum(m1), c = wave_sum(m2);
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        scratch[wid] = a;
        scratch[BLOCK / WAVE + wid] = c;
      }
      __syncthreads();
      m1 = 0.f; m2 = 0.f;
#pragma unroll
      for (int i = 0; i < BLOCK / WAVE; ++i) {
        m1 += scratch[i];
        m2 += scratch[BLOCK / WAVE + i];
      }
    }
    m1 /= D;
    m2 /= D;
    for (int i = threadIdx.x * 8; i < D; i += BLOCK * 8) {
      f8 xv = load8f(xr + i), dyv = load8f(dyr + i), wv = load8f(w + i);
      f8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = (xv.v[j] - mu) * r;
        out.v[j] = r * (wv.v[j] * dyv.v[j] - m1 - xhat * m2);
      }
      store8f(dxr + i, out);
    }
    __syncthreads();
  }
}

template <int NC>
__global__ void rmsnorm_bwd_bf16_reg(const unsigned short* __restrict__ dy,
                                     const unsigned short* __restrict__ x,
                                     const unsigned short* __restrict__ w,
                                     const float* __restrict__ rstd,
                                     unsigned short* __restrict__ dx,
                                     float* __restrict__ dw_partial,
                                     int rows, int D) {
  __shared__ float scratch[BLOCK / WAVE];
  float acc_dw[NC][8];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc_dw[c][j] = 0.f;

  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + (long)row * D;
    const unsigned short* xr = x + (long)row * D;
    unsigned short* dxr = dx + (long)row * D;
    float r = rstd[row];
    float dot = 0.f;
    f8 xv[NC], dyv[NC], wv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        xv[c] = load8f(xr + i);
        dyv[c] = load8f(dyr + i);
        wv[c] = load8f(w + i);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dot += wv[c].v[j] * dyv[c].v[j] * xv[c].v[j] * r;
      }
    }
    dot = block_sum<BLOCK>(dot, scratch) / D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        f8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = xv[c].v[j] * r;
          out.v[j] = r * (wv[c].v[j] * dyv[c].v[j] - xhat * dot);
          acc_dw[c][j] += dyv[c].v[j] * xhat;
        }
        store8f(dxr + i, out);
      }
    }
    __syncthreads();
  }
  // per-block partial row (coalesced plain stores; summed host-side) —
  // atomicAdd here serializes gridDim-deep per element and was 2x slower
  float* dwp = dw_partial + (long)blockIdx.x * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int i = threadIdx.x * 8 + c * BLOCK * 8;
    if (i < D)
#pragma unroll
      for (int j = 0; j < 8; ++j) dwp[i + j] = acc_dw[c][j];
  }
}

// RES == true also adds the residual-stream grad: the row stored is
// g = bf16(float(bf16(dx)) + g_res), which is what autograd's accumulation of
// the LayerNorm input grad and the residual grad gives.  g_res is loaded in
// the second per-row loop, so it is not held across the block reduction.
// COLSUM == true (needs RES) keeps a third accumulator set: the column sums
// of the stored g, i.e. the bias grad of the linear whose output entered the
// junction.  dw and db accumulate exactly as without RES.
template <int NC, bool RES, bool COLSUM>
__global__ void __launch_bounds__(BLOCK)
layernorm_bwd_bf16_reg(const unsigned short* __restrict__ dy,
                       const unsigned short* __restrict__ x,
                       const unsigned short* __restrict__ w,
                       const float* __restrict__ mean,
                       const float* __restrict__ rstd,
                       const unsigned short* __restrict__ g_res,
                       unsigned short* __restrict__ dx,
                       float* __restrict__ dw_partial,
                       float* __restrict__ db_partial,
                       float* __restrict__ dc_partial,
                       int rows, int D) {
  static_assert(RES || !COLSUM, "COLSUM sums the residual-added grad");
  __shared__ float scratch[2 * BLOCK / WAVE];
  float acc_dw[NC][8], acc_db[NC][8];
  float acc_dc[COLSUM ? NC : 1][8];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc_dw[c][j] = 0.f; acc_db[c][j] = 0.f; }
  if constexpr (COLSUM) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc_dc[c][j] = 0.f;
  }

  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + (long)row * D;
    const unsigned short* xr = x + (long)row * D;
    unsigned short* dxr = dx + (long)row * D;
    float mu = mean[row], r = rstd[row];
    float m1 = 0.f, m2 = 0.f;
    f8 xv[NC], dyv[NC], wv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        xv[c] = load8f(xr + i);
        dyv[c] = load8f(dyr + i);
        wv[c] = load8f(w + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (xv[c].v[j] - mu) * r;
          float wdy = wv[c].v[j] * dyv[c].v[j];
          m1 += wdy;
          m2 += wdy * xhat;
        }
      }
    }
    {
      const int wid = threadIdx.x / WAVE;
      float a = wave_sum(m1), cgr = wave_sum(m2);
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        scratch[wid] = a;
        scratch[BLOCK / WAVE + wid] = cgr;
      }
      __syncthreads();
      m1 = 0.f; m2 = 0.f;
#pragma unroll
      for (int i = 0; i < BLOCK / WAVE; ++i) {
        m1 += scratch[i];
        m2 += scratch[BLOCK / WAVE + i];
      }
    }
    m1 /= D;
    m2 /= D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D) {
        f8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (xv[c].v[j] - mu) * r;
          out.v[j] = r * (wv[c].v[j] * dyv[c].v[j] - m1 - xhat * m2);
          acc_dw[c][j] += dyv[c].v[j] * xhat;
          acc_db[c][j] += dyv[c].v[j];
        }
        if constexpr (RES) {
          f8 gr = load8f(g_res + (long)row * D + i);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            out.v[j] = bf2f(f2bf(out.v[j])) + gr.v[j];
            if constexpr (COLSUM) acc_dc[c][j] += bf2f(f2bf(out.v[j]));
          }
        }
        store8f(dxr + i, out);
      }
    }
    __syncthreads();
  }
  float* dwp = dw_partial + (long)blockIdx.x * D;
  float* dbp = db_partial + (long)blockIdx.x * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int i = threadIdx.x * 8 + c * BLOCK * 8;
    if (i < D)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dwp[i + j] = acc_dw[c][j];
        dbp[i + j] = acc_db[c][j];
      }
  }
  if constexpr (COLSUM) {
    float* dcp = dc_partial + (long)blockIdx.x * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int i = threadIdx.x * 8 + c * BLOCK * 8;
      if (i < D)
#pragma unroll
        for (int j = 0; j < 8; ++j) dcp[i + j] = acc_dc[c][j];
    }
  }
}

}  // namespace

// ------------------------------------------------------------------ C++ API

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int D = x.size(-1);
  TORCH_CHECK(D <= MAX_D, "D too large");
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(pick_grid(rows)), block(BLOCK);
  if (x.scalar_type() == torch::kBFloat16 && D % 8 == 0) {
    hipLaunchKernelGGL(rmsnorm_fwd_bf16v8, grid, block, 0, stream,
                       (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)w.data_ptr(),
                       (unsigned short*)y.data_ptr(), rstd.data_ptr<float>(),
                       (int)rows, D, (float)eps);
  } else if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<bf16_t>, grid, block, 0, stream,
                       (const bf16_t*)x.data_ptr(), (const bf16_t*)w.data_ptr(),
                       (bf16_t*)y.data_ptr(), rstd.data_ptr<float>(),
                       (int)rows, D, (float)eps);
  } else {
    TORCH_CHECK(x.scalar_type() == torch::kFloat, "bf16/f32 only");
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<float>, grid, block, 0, stream,
                       x.data_ptr<float>(), w.data_ptr<float>(),
                       y.data_ptr<float>(), rstd.data_ptr<float>(),
                       (int)rows, D, (float)eps);
  }
  HIP_CHECK_LAST();
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor rstd) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(pick_grid(rows)), block(BLOCK);
  const bool reg_path = x.scalar_type() == torch::kBFloat16 &&
      D % 8 == 0 && D <= 4 * BLOCK * 8;
  if (reg_path) {
    auto dw_partial = torch::empty({(long)grid.x, (long)D},
                                   x.options().dtype(torch::kFloat));
    int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define RMS_REG(NC)                                                          \
    hipLaunchKernelGGL(rmsnorm_bwd_bf16_reg<NC>, grid, block, 0, stream,     \
                       (const unsigned short*)dy.data_ptr(),                 \
                       (const unsigned short*)x.data_ptr(),                  \
                       (const unsigned short*)w.data_ptr(),                  \
                       rstd.data_ptr<float>(),                               \
                       (unsigned short*)dx.data_ptr(),                       \
                       dw_partial.data_ptr<float>(), (int)rows, D)
    if (nc == 1) RMS_REG(1); else if (nc == 2) RMS_REG(2);
    else if (nc == 3) RMS_REG(3); else RMS_REG(4);
#undef RMS_REG
    HIP_CHECK_LAST();
    return {dx, dw_partial.sum(0).to(w.scalar_type())};
  }
  // dx from the row kernels, dw from the fixed-order column kernel
  auto dw = torch::empty({D}, x.options().dtype(torch::kFloat));
  dim3 grid_dw((D + DW_COLS - 1) / DW_COLS);
  if (x.scalar_type() == torch::kBFloat16) {
    if (D % 8 == 0) {
      hipLaunchKernelGGL(rmsnorm_bwd_bf16v8, grid, block, 0, stream,
                         (const unsigned short*)dy.data_ptr(),
                         (const unsigned short*)x.data_ptr(),
                         (const unsigned short*)w.data_ptr(),
                         rstd.data_ptr<float>(),
                         (unsigned short*)dx.data_ptr(), (int)rows, D);
    } else {
      hipLaunchKernelGGL(rmsnorm_bwd_kernel<bf16_t>, grid, block, 0, stream,
                         (const bf16_t*)dy.data_ptr(),
                         (const bf16_t*)x.data_ptr(),
                         (const bf16_t*)w.data_ptr(), rstd.data_ptr<float>(),
                         (bf16_t*)dx.data_ptr(), (int)rows, D);
    }
    hipLaunchKernelGGL((norm_bwd_dwdb_kernel<bf16_t, false>), grid_dw, block,
                       0, stream, (const bf16_t*)dy.data_ptr(),
                       (const bf16_t*)x.data_ptr(), (const float*)nullptr,
                       rstd.data_ptr<float>(), dw.data_ptr<float>(),
                       (float*)nullptr, (int)rows, D);
  } else {
    TORCH_CHECK(x.scalar_type() == torch::kFloat, "bf16/f32 only");
    hipLaunchKernelGGL(rmsnorm_bwd_kernel<float>, grid, block, 0, stream,
                       dy.data_ptr<float>(), x.data_ptr<float>(),
                       w.data_ptr<float>(), rstd.data_ptr<float>(),
                       dx.data_ptr<float>(), (int)rows, D);
    hipLaunchKernelGGL((norm_bwd_dwdb_kernel<float, false>), grid_dw, block,
                       0, stream, dy.data_ptr<float>(), x.data_ptr<float>(),
                       (const float*)nullptr, rstd.data_ptr<float>(),
                       dw.data_ptr<float>(), (float*)nullptr, (int)rows, D);
  }
  HIP_CHECK_LAST();
  return {dx, dw.to(w.scalar_type())};
}

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int D = x.size(-1);
  TORCH_CHECK(D <= MAX_D, "D too large");
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat));
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(pick_grid(rows)), block(BLOCK);
  if (x.scalar_type() == torch::kBFloat16 && D % 8 == 0) {
    // MAX_D = 8 chunks of BLOCK * 8
    const int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define LN_FWD(NC)                                                           \
    hipLaunchKernelGGL((layernorm_fwd_bf16v8<NC, false>), grid, block, 0,    \
                       stream, (const unsigned short*)x.data_ptr(),          \
                       (const unsigned short*)nullptr,                       \
                       (const unsigned short*)nullptr,                       \
                       (const unsigned short*)w.data_ptr(),                  \
                       (const unsigned short*)b.data_ptr(),                  \
                       (unsigned short*)nullptr,                             \
                       (unsigned short*)y.data_ptr(),                        \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                       (int)rows, D, (float)eps)
    if (nc == 1) LN_FWD(1); else if (nc == 2) LN_FWD(2);
    else if (nc <= 4) LN_FWD(4); else LN_FWD(8);
#undef LN_FWD
  } else if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(layernorm_fwd_kernel<bf16_t>, grid, block, 0, stream,
                       (const bf16_t*)x.data_ptr(), (const bf16_t*)w.data_ptr(),
                       (const bf16_t*)b.data_ptr(), (bf16_t*)y.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       (int)rows, D, (float)eps);
  } else {
    TORCH_CHECK(x.scalar_type() == torch::kFloat, "bf16/f32 only");
    hipLaunchKernelGGL(layernorm_fwd_kernel<float>, grid, block, 0, stream,
                       x.data_ptr<float>(), w.data_ptr<float>(),
                       b.data_ptr<float>(), y.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       (int)rows, D, (float)eps);
  }
  HIP_CHECK_LAST();
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(pick_grid(rows)), block(BLOCK);
  const bool reg_path = x.scalar_type() == torch::kBFloat16 &&
      D % 8 == 0 && D <= 4 * BLOCK * 8;
  if (reg_path) {
    auto dw_partial = torch::empty({(long)grid.x, (long)D},
                                   x.options().dtype(torch::kFloat));
    auto db_partial = torch::empty({(long)grid.x, (long)D},
                                   x.options().dtype(torch::kFloat));
    int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define LN_REG(NC)                                                           \
    hipLaunchKernelGGL((layernorm_bwd_bf16_reg<NC, false, false>), grid,     \
                       block, 0, stream,                                     \
                       (const unsigned short*)dy.data_ptr(),                 \
                       (const unsigned short*)x.data_ptr(),                  \
                       (const unsigned short*)w.data_ptr(),                  \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                       (const unsigned short*)nullptr,                       \
                       (unsigned short*)dx.data_ptr(),                       \
                       dw_partial.data_ptr<float>(),                         \
                       db_partial.data_ptr<float>(), (float*)nullptr,        \
                       (int)rows, D)
    if (nc == 1) LN_REG(1); else if (nc == 2) LN_REG(2);
    else if (nc == 3) LN_REG(3); else LN_REG(4);
#undef LN_REG
    HIP_CHECK_LAST();
    return {dx, dw_partial.sum(0).to(w.scalar_type()),
            db_partial.sum(0).to(w.scalar_type())};
  }
  // dx from the row kernels, dw and db from the fixed-order column kernel
  auto dw = torch::empty({D}, x.options().dtype(torch::kFloat));
  auto db = torch::empty({D}, x.options().dtype(torch::kFloat));
  dim3 grid_dw((D + DW_COLS - 1) / DW_COLS);
  if (x.scalar_type() == torch::kBFloat16) {
    if (D % 8 == 0) {
      hipLaunchKernelGGL(layernorm_bwd_bf16v8, grid, block, 0, stream,
                         (const unsigned short*)dy.data_ptr(),
                         (const unsigned short*)x.data_ptr(),
                         (const unsigned short*)w.data_ptr(),
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),
                         (unsigned short*)dx.data_ptr(), (int)rows, D);
    } else {
      hipLaunchKernelGGL(layernorm_bwd_kernel<bf16_t>, grid, block, 0, stream,
                         (const bf16_t*)dy.data_ptr(),
                         (const bf16_t*)x.data_ptr(),
                         (const bf16_t*)w.data_ptr(), mean.data_ptr<float>(),
                         rstd.data_ptr<float>(), (bf16_t*)dx.data_ptr(),
                         (int)rows, D);
    }
    hipLaunchKernelGGL((norm_bwd_dwdb_kernel<bf16_t, true>), grid_dw, block,
                       0, stream, (const bf16_t*)dy.data_ptr(),
                       (const bf16_t*)x.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), dw.data_ptr<float>(),
                       db.data_ptr<float>(), (int)rows, D);
  } else {
    TORCH_CHECK(x.scalar_type() == torch::kFloat, "bf16/f32 only");
    hipLaunchKernelGGL(layernorm_bwd_kernel<float>, grid, block, 0, stream,
                       dy.data_ptr<float>(), x.data_ptr<float>(),
                       w.data_ptr<float>(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), dx.data_ptr<float>(),
                       (int)rows, D);
    hipLaunchKernelGGL((norm_bwd_dwdb_kernel<float, true>), grid_dw, block,
                       0, stream, dy.data_ptr<float>(), x.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       dw.data_ptr<float>(), db.data_ptr<float>(),
                       (int)rows, D);
  }
  HIP_CHECK_LAST();
  return {dx, dw.to(w.scalar_type()), db.to(w.scalar_type())};
}

// ------------------------------------------- fused residual-stream junction

namespace {

// the fused kernels cover what the register path covers: bf16, contiguous,
// D % 8 == 0, D <= 4 chunks of BLOCK * 8
constexpr int FUSED_LN_MAX_D = 4 * BLOCK * 8;

int fused_ln_width(const char* fn, const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 &&
                  x.is_contiguous() && x.dim() >= 1 && aligned16(x),
              fn, ": needs a contiguous, 16-byte aligned bf16 device tensor");
  const int D = x.size(-1);
  TORCH_CHECK(D > 0 && D % 8 == 0 && D <= FUSED_LN_MAX_D, fn,
              ": last dim must be a multiple of 8 up to ", FUSED_LN_MAX_D,
              ", got ", D);
  return D;
}

}  // namespace

// widest last dim the fused LayerNorm kernels take (the Python gate asks)
int64_t fused_ln_max_d() { return FUSED_LN_MAX_D; }

// (x_new, h, mean, rstd) of h = layer_norm(x_new), x_new = x_res + (y + bias),
// in one pass; bit-identical to the unfused ops.  bias may be absent.
std::vector<torch::Tensor> bias_residual_layernorm_fwd(
    torch::Tensor y, c10::optional<torch::Tensor> bias, torch::Tensor x_res,
    torch::Tensor ln_w, torch::Tensor ln_b, double eps) {
  const char* fn = "bias_residual_layernorm_fwd";
  const int D = fused_ln_width(fn, x_res);
  check_bf16_rows(fn, "y", y, x_res);
  check_bf16_vec(fn, "ln_w", ln_w, x_res, D);
  check_bf16_vec(fn, "ln_b", ln_b, x_res, D);
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias) check_bf16_vec(fn, "bias", *bias, x_res, D);
  const long rows = x_res.numel() / D;
  auto x_new = torch::empty_like(x_res);
  auto h = torch::empty_like(x_res);
  auto mean = torch::empty({rows}, x_res.options().dtype(torch::kFloat));
  auto rstd = torch::empty({rows}, x_res.options().dtype(torch::kFloat));
  if (rows == 0) return {x_new, h, mean, rstd};
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(pick_grid(rows)), block(BLOCK);
  const int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define LN_FWD_RES(NC)                                                       \
  hipLaunchKernelGGL((layernorm_fwd_bf16v8<NC, true>), grid, block, 0,       \
                     stream, (const unsigned short*)x_res.data_ptr(),        \
                     (const unsigned short*)y.data_ptr(),                    \
                     has_bias ? (const unsigned short*)bias->data_ptr()      \
                              : (const unsigned short*)nullptr,              \
                     (const unsigned short*)ln_w.data_ptr(),                 \
                     (const unsigned short*)ln_b.data_ptr(),                 \
                     (unsigned short*)x_new.data_ptr(),                      \
                     (unsigned short*)h.data_ptr(),                          \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                     (int)rows, D, (float)eps)
  // same chunk counts as layernorm_fwd, so the same reduction order
  if (nc == 1) LN_FWD_RES(1); else if (nc == 2) LN_FWD_RES(2);
  else LN_FWD_RES(4);
#undef LN_FWD_RES
  HIP_CHECK_LAST();
  return {x_new, h, mean, rstd};
}

// (g, partial): g = layer-norm input grad + g_res, and partial, an fp32
// (2 or 3, grid, D) tensor of per-block column sums: partial[0], [1] and,
// with want_colsum, [2] summed over their dim 0 give dw, db and colsum(g).
// The caller finishes with one sum(0) PER SLICE: a slice is reduced exactly
// as layernorm_bwd's own partial is, which keeps dw and db bit-identical to
// it; one sum(1) over the whole tensor does not.
std::vector<torch::Tensor> layernorm_bwd_residual(
    torch::Tensor dh, torch::Tensor x, torch::Tensor w, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor g_res, bool want_colsum) {
  const char* fn = "layernorm_bwd_residual";
  const int D = fused_ln_width(fn, x);
  check_bf16_rows(fn, "dh", dh, x);
  check_bf16_rows(fn, "g_res", g_res, x);
  check_bf16_vec(fn, "w", w, x, D);
  const long rows = x.numel() / D;
  TORCH_CHECK(mean.is_cuda() && rstd.is_cuda() &&
                  mean.scalar_type() == torch::kFloat &&
                  rstd.scalar_type() == torch::kFloat &&
                  mean.is_contiguous() && rstd.is_contiguous() &&
                  mean.numel() == rows && rstd.numel() == rows,
              fn, ": mean and rstd must be contiguous fp32 with one value "
              "per row (", rows, ")");
  auto g = torch::empty_like(x);
  dim3 grid(pick_grid(rows)), block(BLOCK);
  const long np = want_colsum ? 3 : 2;
  auto opts = x.options().dtype(torch::kFloat);
  if (rows == 0) return {g, torch::zeros({np, 1, (long)D}, opts)};
  auto partial = torch::empty({np, (long)grid.x, (long)D}, opts);
  float* pp = partial.data_ptr<float>();
  const long pstride = (long)grid.x * D;
  auto stream = at::cuda::getCurrentHIPStream();
  const int nc = (D + BLOCK * 8 - 1) / (BLOCK * 8);
#define LN_REG_RES(NC, CS)                                                   \
  hipLaunchKernelGGL((layernorm_bwd_bf16_reg<NC, true, CS>), grid, block, 0, \
                     stream, (const unsigned short*)dh.data_ptr(),           \
                     (const unsigned short*)x.data_ptr(),                    \
                     (const unsigned short*)w.data_ptr(),                    \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                     (const unsigned short*)g_res.data_ptr(),                \
                     (unsigned short*)g.data_ptr(), pp, pp + pstride,        \
                     CS ? pp + 2 * pstride : (float*)nullptr, (int)rows, D)
#define LN_REG_RES_NC(NC)                                                    \
  do {                                                                       \
    if (want_colsum) LN_REG_RES(NC, true); else LN_REG_RES(NC, false);       \
  } while (0)
  if (nc == 1) LN_REG_RES_NC(1); else if (nc == 2) LN_REG_RES_NC(2);
  else if (nc == 3) LN_REG_RES_NC(3); else LN_REG_RES_NC(4);
#undef LN_REG_RES_NC
#undef LN_REG_RES
  HIP_CHECK_LAST();
  return {g, partial};
}
