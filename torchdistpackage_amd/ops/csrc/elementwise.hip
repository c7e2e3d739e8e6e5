// Fused elementwise / reduction kernels for gfx950:
//   - bias_gelu fwd/bwd (tanh GELU, GPT-2 convention) — fuses the reference's
//     nn.GELU after fc1 (/root/reference/.../tensor_parallel/mlp.py:30-32)
//   - fused AdamW step on flat fp32 shards (replaces torch.optim.AdamW.step
//     per-tensor loop, reference zero_optim.py:265)
//   - EMA update (reference sharded_ema.py:29 mul_/add_ pair -> one pass)
//   - l2norm_sq + inplace scale (grad clip, reference clip_grad_parallel.py)
//
// All memory-bound: grid-stride loops, 256-thread blocks, bf16 vectorized as
// ushort4/bf16x8 (8-16 B per lane) where applicable, f32 math.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "fused_checks.h"

namespace {

constexpr int BLOCK = 256;
constexpr float GELU_C = 0.7978845608028654f;   // sqrt(2/pi)
constexpr float GELU_A = 0.044715f;

// tanh via the hardware exp2 unit: tanh(x) = 1 - 2/(exp2(x*2*log2e)+1).
// Overflow saturates the right way (exp2->inf -> rcp->0 -> +1; exp2->0 -> -1)
// so no range branches are needed; ulp-exact at bf16 output precision and
// ~5x fewer instructions than libm tanhf (which rate-limited the fused
// bias+GELU kernels below ~3.3 TB/s; HBM roofline is ~6).
DEVINL float tanh_fast(float x) {
  float e = __builtin_amdgcn_exp2f(x * 2.885390082f);  // 2*log2(e)
  return 1.f - 2.f / (e + 1.f);
}

DEVINL float gelu_f(float u) {
  float t = tanh_fast(GELU_C * (u + GELU_A * u * u * u));
  return 0.5f * u * (1.f + t);
}

DEVINL float gelu_df(float u) {
  float u2 = u * u;
  float t = tanh_fast(GELU_C * (u + GELU_A * u * u2));
  return 0.5f * (1.f + t) +
         0.5f * u * (1.f - t * t) * GELU_C * (1.f + 3.f * GELU_A * u2);
}

// gelu_df for bias_gelu_bwd_bf16 (vector path and tail), with the contraction
// written out: which multiply fuses with which add is otherwise the
// compiler's choice per use (with the column sums added to the loop it fused
// one element pair differently, and dx moved by a bf16 ulp on ~1e-4 of the
// elements where the two terms cancel).  This is the sequence the plain
// kernel has always compiled to, so its dx is unchanged.
DEVINL float gelu_df_pinned(float u) {
#pragma clang fp contract(off)
  float u2 = u * u;
  float t = tanh_fast(GELU_C * fmaf(GELU_A * u, u2, u));
  float k = fmaf(u2, 3.f * GELU_A, 1.f);
  float m = 0.5f * u * fmaf(-t, t, 1.f) * GELU_C * k;
  return fmaf(1.f + t, 0.5f, m);
}

// -------- bias_gelu: x (rows, D) bf16, bias (D) bf16 (or empty) ----------

__global__ void bias_gelu_fwd_bf16(const unsigned short* __restrict__ x,
                                   const unsigned short* __restrict__ bias,
                                   unsigned short* __restrict__ y,
                                   long n, int D, int has_bias) {
  long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * 8;
  long stride = (long)gridDim.x * BLOCK * 8;
  for (long i = i0; i < n; i += stride) {
    if (i + 8 <= n) {
      bf16x8 xv = *(const bf16x8*)(x + i);
      // D % 8 == 0 guaranteed by caller for the vector path
      bf16x8 bv;
      if (has_bias) bv = *(const bf16x8*)(bias + (int)(i % D));
      const unsigned short* xs = (const unsigned short*)&xv;
      const unsigned short* bs = (const unsigned short*)&bv;
      bf16x8 out;
      unsigned short* os = (unsigned short*)&out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float b = has_bias ? bf2f(bs[j]) : 0.f;
        os[j] = f2bf(gelu_f(bf2f(xs[j]) + b));
      }
      *(bf16x8*)(y + i) = out;
    } else {
      for (long j = i; j < n; ++j) {
        float b = has_bias ? bf2f(bias[j % D]) : 0.f;
        y[j] = f2bf(gelu_f(bf2f(x[j]) + b));
      }
    }
  }
}

// COLSUM == true also gives the column sums of the dx it stores (the fc1
// bias grad), so nothing has to read dx back.  It is the same flat
// grid-stride loop, launched with a grid whose stride gridDim.x * BLOCK * 8
// is a multiple of D: then a thread stays on the same 8 columns in every
// iteration, its rows are (i0 / D) + k * (stride / D), and it keeps 8 fp32
// sums of the bf16-rounded dx it stored.  The sums go to partial[i0 ..
// i0 + 8), which makes ``partial`` a (stride / D, D) matrix of per-row-lane
// column sums; the caller finishes with a sum over dim 0.  The element
// arithmetic is one piece of code for both forms, so dx does not depend on
// which one ran.
template <bool COLSUM>
__global__ void bias_gelu_bwd_bf16(const unsigned short* __restrict__ dy,
                                   const unsigned short* __restrict__ x,
                                   const unsigned short* __restrict__ bias,
                                   unsigned short* __restrict__ dx,
                                   float* __restrict__ partial,
                                   long n, int D, int has_bias) {
  long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * 8;
  long stride = (long)gridDim.x * BLOCK * 8;
  float acc[8];
  if constexpr (COLSUM) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  }
  for (long i = i0; i < n; i += stride) {
    if (i + 8 <= n) {
      bf16x8 xv = *(const bf16x8*)(x + i);
      bf16x8 gv = *(const bf16x8*)(dy + i);
      bf16x8 bv;
      if (has_bias) bv = *(const bf16x8*)(bias + (int)(i % D));
      const unsigned short* xs = (const unsigned short*)&xv;
      const unsigned short* gs = (const unsigned short*)&gv;
      const unsigned short* bs = (const unsigned short*)&bv;
      bf16x8 out;
      unsigned short* os = (unsigned short*)&out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float b = has_bias ? bf2f(bs[j]) : 0.f;
        os[j] = f2bf(bf2f(gs[j]) * gelu_df_pinned(bf2f(xs[j]) + b));
        if constexpr (COLSUM) acc[j] += bf2f(os[j]);
      }
      *(bf16x8*)(dx + i) = out;
    } else {
      // never with COLSUM: its caller requires D % 8 == 0, so n % 8 == 0
      for (long j = i; j < n; ++j) {
        float b = has_bias ? bf2f(bias[j % D]) : 0.f;
        dx[j] = f2bf(bf2f(dy[j]) * gelu_df_pinned(bf2f(x[j]) + b));
      }
    }
  }
  if constexpr (COLSUM) {
    *(float4*)(partial + i0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *(float4*)(partial + i0 + 4) =
        make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

__global__ void bias_gelu_fwd_f32(const float* __restrict__ x,
                                  const float* __restrict__ bias,
                                  float* __restrict__ y,
                                  long n, int D, int has_bias) {
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  for (long i = i0; i < n; i += stride) {
    float b = has_bias ? bias[i % D] : 0.f;
    y[i] = gelu_f(x[i] + b);
  }
}

__global__ void bias_gelu_bwd_f32(const float* __restrict__ dy,
                                  const float* __restrict__ x,
                                  const float* __restrict__ bias,
                                  float* __restrict__ dx,
                                  long n, int D, int has_bias) {
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  for (long i = i0; i < n; i += stride) {
    float b = has_bias ? bias[i % D] : 0.f;
    dx[i] = dy[i] * gelu_df(x[i] + b);
  }
}

// out = bf16(x + bf16(y + bias)): the Row-parallel bias add and the residual
// add that follows it, in one pass with the two roundings of the two passes.
// bias may be null (then out = bf16(x + y)).  D % 8 == 0.
__global__ void bias_residual_add_bf16(const unsigned short* __restrict__ y,
                                       const unsigned short* __restrict__ bias,
                                       const unsigned short* __restrict__ x,
                                       unsigned short* __restrict__ out,
                                       long n, int D) {
  long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * 8;
  long stride = (long)gridDim.x * BLOCK * 8;
  for (long i = i0; i < n; i += stride) {   // n % 8 == 0
    bf16x8 yv = *(const bf16x8*)(y + i);
    bf16x8 xv = *(const bf16x8*)(x + i);
    bf16x8 bv;
    if (bias != nullptr) bv = *(const bf16x8*)(bias + (int)(i % D));
    const unsigned short* ys = (const unsigned short*)&yv;
    const unsigned short* xs = (const unsigned short*)&xv;
    const unsigned short* bs = (const unsigned short*)&bv;
    bf16x8 ov;
    unsigned short* os = (unsigned short*)&ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = bf2f(ys[j]);
      if (bias != nullptr) t = bf2f(f2bf(t + bf2f(bs[j])));
      os[j] = f2bf(bf2f(xs[j]) + t);
    }
    *(bf16x8*)(out + i) = ov;
  }
}

// -------- fused AdamW on flat fp32 tensors -------------------------------

// The step-dependent coefficients, each computed in double and rounded to
// fp32 ONCE (forming 1.f - beta2 in fp32 with beta2 = 0.999 is 1.3e-5 off).
// They come either from the host (adam_coef_host) or from device memory,
// written by adam_prelude_kernel (the hipGraph-capturable optimizer).
struct AdamCoef {
  float omb1;       // 1 - beta1
  float omb2;       // 1 - beta2
  float bc2;        // 1 - beta2^step
  float step_size;  // lr / (1 - beta1^step)
  float decay;      // 1 - lr * wd
};
constexpr int ADAM_NCOEF = 5;   // floats per group in the device table
constexpr int ADAM_NHYP = 4;    // doubles per group: lr, beta1, beta2, wd

DEVINL AdamCoef adam_coef_load(AdamCoef c, const float* __restrict__ cdev) {
  if (cdev != nullptr) {
    c.omb1 = cdev[0];
    c.omb2 = cdev[1];
    c.bc2 = cdev[2];
    c.step_size = cdev[3];
    c.decay = cdev[4];
  }
  return c;
}

DEVINL void adam_elem(float& p, float& m, float& v, float g, float beta1,
                      float beta2, float eps, const AdamCoef& c) {
  float mi = m * beta1 + g * c.omb1;
  float vi = v * beta2 + g * g * c.omb2;
  m = mi;
  v = vi;
  p = p * c.decay - c.step_size * mi / (sqrtf(vi / c.bc2) + eps);
}

// One block: advances the device step counter and writes every group's
// coefficients for the update kernels launched after it on the same stream.
// Being a kernel, it is recorded by a hipGraph capture and runs again on
// every replay, so the bias corrections follow the real step count.
__global__ void adam_prelude_kernel(long* __restrict__ step,
                                    const double* __restrict__ hyp,
                                    float* __restrict__ coef, int ngroups) {
  const long t = *step + 1;
  __syncthreads();                 // every thread has read the old count
  for (int g = threadIdx.x; g < ngroups; g += blockDim.x) {
    const double lr = hyp[g * ADAM_NHYP + 0];
    const double b1 = hyp[g * ADAM_NHYP + 1];
    const double b2 = hyp[g * ADAM_NHYP + 2];
    const double wd = hyp[g * ADAM_NHYP + 3];
    const double bc1 = 1.0 - pow(b1, (double)t);
    const double bc2 = 1.0 - pow(b2, (double)t);
    float* c = coef + g * ADAM_NCOEF;
    c[0] = (float)(1.0 - b1);
    c[1] = (float)(1.0 - b2);
    c[2] = (float)bc2;
    c[3] = (float)(lr / bc1);
    c[4] = (float)(1.0 - lr * wd);
  }
  if (threadIdx.x == 0) *step = t;
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v,
                             long n, float beta1, float beta2, float eps,
                             AdamCoef ch, const float* __restrict__ cdev) {
  const AdamCoef c = adam_coef_load(ch, cdev);
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  for (long i = i0; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, mi, vi, g[i], beta1, beta2, eps, c);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// -------- EMA: ema = d*ema + (1-d)*p (f32 ema; f32 OR bf16 p) ------------

// vectorized 4-wide (the v10 adamw lesson: scalar dword accesses cap the
// HBM-bound kernels well below the roofline); scalar tail for n % 4
__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ p,
                           long n, float decay, float omd, int vec4) {
  const long n4 = vec4 ? (n >> 2) : 0;
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  for (long i = i0; i < n4; i += stride) {
    float4 e = *(const float4*)(ema + i * 4);
    float4 v = *(const float4*)(p + i * 4);
    e.x = decay * e.x + omd * v.x;
    e.y = decay * e.y + omd * v.y;
    e.z = decay * e.z + omd * v.z;
    e.w = decay * e.w + omd * v.w;
    *(float4*)(ema + i * 4) = e;
  }
  for (long i = n4 * 4 + i0; i < n; i += stride)
    ema[i] = decay * ema[i] + omd * p[i];
}

// -------- l2 norm squared (any dtype -> f32 scalar) ----------------------

// Each block writes its partial; l2norm_final_kernel adds them in a fixed
// order.  (A float atomicAdd per block summed them in arrival order, so the
// result, and with it the clip coefficient, changed from call to call.)
template <typename T>
__global__ void l2norm_kernel(const T* __restrict__ x,
                              float* __restrict__ partial, long n) {
  __shared__ float lds[BLOCK / WAVE];
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  float acc = 0.f;
  for (long i = i0; i < n; i += stride) {
    float v;
    if constexpr (sizeof(T) == 2) v = bf2f(((const unsigned short*)x)[i]);
    else v = ((const float*)x)[i];
    acc += v * v;
  }
  acc = block_sum<BLOCK>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void l2norm_final_kernel(const float* __restrict__ partial,
                                    float* __restrict__ out, int nparts) {
  __shared__ float lds[BLOCK / WAVE];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += BLOCK) acc += partial[i];
  acc = block_sum<BLOCK>(acc, lds);
  if (threadIdx.x == 0) *out = acc;
}

template <typename T>
__global__ void scale_kernel(T* __restrict__ x, long n, float s) {
  long i0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * BLOCK;
  for (long i = i0; i < n; i += stride) {
    if constexpr (sizeof(T) == 2) {
      unsigned short* p = (unsigned short*)x;
      p[i] = f2bf(bf2f(p[i]) * s);
    } else {
      ((float*)x)[i] *= s;
    }
  }
}

int ew_grid(long n, int per_thread = 1) {
  long blocks = (n + (long)BLOCK * per_thread - 1) / ((long)BLOCK * per_thread);
  return (int)(blocks > 2048 ? 2048 : (blocks > 0 ? blocks : 1));
}

AdamCoef adam_coef_host(long step, double lr, double beta1, double beta2,
                        double wd) {
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  AdamCoef c;
  c.omb1 = (float)(1.0 - beta1);
  c.omb2 = (float)(1.0 - beta2);
  c.bc2 = (float)bc2;
  c.step_size = (float)(lr / bc1);
  c.decay = (float)(1.0 - lr * wd);
  return c;
}

// the flat kernel indexes all four tensors 0..p.numel() as dense fp32
void check_adamw_flat(const torch::Tensor& p, const torch::Tensor& g,
                      const torch::Tensor& m, const torch::Tensor& v) {
  const torch::Tensor* ts[4] = {&p, &g, &m, &v};
  const char* names[4] = {"p", "g", "m", "v"};
  for (int i = 0; i < 4; ++i) {
    TORCH_CHECK(ts[i]->is_cuda() && ts[i]->scalar_type() == torch::kFloat,
                "adamw_step: ", names[i], " must be an fp32 device tensor");
    TORCH_CHECK(ts[i]->is_contiguous(), "adamw_step: ", names[i],
                " must be contiguous");
    TORCH_CHECK(ts[i]->numel() == p.numel(), "adamw_step: ", names[i],
                " has ", ts[i]->numel(), " elements, p has ", p.numel());
    TORCH_CHECK(ts[i]->get_device() == p.get_device(), "adamw_step: ",
                names[i], " is on another device than p");
  }
}

void check_adam_coef(const torch::Tensor& coef, const torch::Tensor& like) {
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == torch::kFloat &&
              coef.is_contiguous() && coef.numel() == ADAM_NCOEF &&
              coef.get_device() == like.get_device(),
              "adamw: coef must be ", ADAM_NCOEF,
              " contiguous fp32 values on the params' device");
}

}  // namespace

// ------------------------------------------------------------------ C++ API

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  auto y = torch::empty_like(x);
  long n = x.numel();
  int D = x.size(-1);
  int has_bias = bias.numel() > 0 ? 1 : 0;
  auto stream = at::cuda::getCurrentHIPStream();
  if (x.scalar_type() == torch::kBFloat16) {
    TORCH_CHECK(!has_bias || (D % 8 == 0), "D must be multiple of 8");
    hipLaunchKernelGGL(bias_gelu_fwd_bf16, dim3(ew_grid(n, 8)), dim3(BLOCK), 0,
                       stream, (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)bias.data_ptr(),
                       (unsigned short*)y.data_ptr(), n, D, has_bias);
  } else {
    hipLaunchKernelGGL(bias_gelu_fwd_f32, dim3(ew_grid(n)), dim3(BLOCK), 0,
                       stream, x.data_ptr<float>(), bias.data_ptr<float>(),
                       y.data_ptr<float>(), n, D, has_bias);
  }
  HIP_CHECK_LAST();
  return y;
}

torch::Tensor bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                            torch::Tensor bias) {
  auto dx = torch::empty_like(x);
  long n = x.numel();
  int D = x.size(-1);
  int has_bias = bias.numel() > 0 ? 1 : 0;
  auto stream = at::cuda::getCurrentHIPStream();
  if (x.scalar_type() == torch::kBFloat16) {
    TORCH_CHECK(!has_bias || (D % 8 == 0), "D must be multiple of 8");
    hipLaunchKernelGGL(bias_gelu_bwd_bf16<false>, dim3(ew_grid(n, 8)),
                       dim3(BLOCK), 0, stream,
                       (const unsigned short*)dy.data_ptr(),
                       (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)bias.data_ptr(),
                       (unsigned short*)dx.data_ptr(), (float*)nullptr, n, D,
                       has_bias);
  } else {
    hipLaunchKernelGGL(bias_gelu_bwd_f32, dim3(ew_grid(n)), dim3(BLOCK), 0,
                       stream, dy.data_ptr<float>(), x.data_ptr<float>(),
                       bias.data_ptr<float>(), dx.data_ptr<float>(),
                       n, D, has_bias);
  }
  HIP_CHECK_LAST();
  return dx;
}

namespace {
// grid of the COLSUM form of bias_gelu_bwd_bf16: a multiple of
// q = D / gcd(D, BLOCK * 8) blocks, so that the grid's stride is a multiple
// of D; as many as the flat kernel would get (at most 2048), at least q.
// 0 if q itself is above 2048 blocks.
long colsum_grid(long n, int D) {
  long a = D, b = (long)BLOCK * 8;
  while (b) { long t = a % b; a = b; b = t; }
  const long q = D / a;
  if (q > 2048) return 0;
  const long want = ew_grid(n, 8);
  return want < q ? q : want / q * q;
}
}  // namespace

// (dx, partial): dx as bias_gelu_bwd, and fp32 (lanes, D) partial column sums
// of dx; partial.sum(0) is the bias grad.  bf16 with a bias only, and D must
// pass bias_gelu_bwd_colsum_ok.
std::vector<torch::Tensor> bias_gelu_bwd_colsum(torch::Tensor dy,
                                                torch::Tensor x,
                                                torch::Tensor bias) {
  const char* fn = "bias_gelu_bwd_colsum";
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 &&
                  x.is_contiguous() && x.dim() >= 1 && aligned16(x),
              fn, ": x must be a contiguous, 16-byte aligned bf16 device "
              "tensor");
  const int D = x.size(-1);
  TORCH_CHECK(D > 0 && D % 8 == 0, fn, ": D must be a multiple of 8, got ", D);
  check_bf16_rows(fn, "dy", dy, x);
  check_bf16_vec(fn, "bias", bias, x, D);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat);
  if (rows == 0) return {dx, torch::zeros({1, (long)D}, opts)};
  // (16384, 8192): 2048 blocks, a (512, 8192) partial of 16 MB against the
  // 268 MB read of dx it replaces
  const long grid = colsum_grid(x.numel(), D);
  TORCH_CHECK(grid > 0, fn, ": no grid of at most 2048 blocks has a stride "
              "that is a multiple of D = ", D);
  auto partial = torch::empty({grid * BLOCK * 8 / D, (long)D}, opts);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(bias_gelu_bwd_bf16<true>, dim3((unsigned)grid),
                     dim3(BLOCK), 0, stream,
                     (const unsigned short*)dy.data_ptr(),
                     (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)bias.data_ptr(),
                     (unsigned short*)dx.data_ptr(),
                     partial.data_ptr<float>(), x.numel(), D, 1);
  HIP_CHECK_LAST();
  return {dx, partial};
}

bool bias_gelu_bwd_colsum_ok(int64_t D) {
  return D > 0 && D % 8 == 0 && colsum_grid(1, (int)D) > 0;
}

// bf16(x_res + bf16(y + bias)) in one pass; bias may be absent.
torch::Tensor bias_residual_add(torch::Tensor y,
                                c10::optional<torch::Tensor> bias,
                                torch::Tensor x_res) {
  const char* fn = "bias_residual_add";
  TORCH_CHECK(x_res.is_cuda() && x_res.scalar_type() == torch::kBFloat16 &&
                  x_res.is_contiguous() && x_res.dim() >= 1 &&
                  aligned16(x_res),
              fn, ": x_res must be a contiguous, 16-byte aligned bf16 device "
              "tensor");
  const int D = x_res.size(-1);
  TORCH_CHECK(D > 0 && D % 8 == 0, fn, ": D must be a multiple of 8, got ", D);
  check_bf16_rows(fn, "y", y, x_res);
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias) check_bf16_vec(fn, "bias", *bias, x_res, D);
  auto out = torch::empty_like(x_res);
  const long n = x_res.numel();
  if (n == 0) return out;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(bias_residual_add_bf16, dim3(ew_grid(n, 8)), dim3(BLOCK),
                     0, stream, (const unsigned short*)y.data_ptr(),
                     has_bias ? (const unsigned short*)bias->data_ptr()
                              : (const unsigned short*)nullptr,
                     (const unsigned short*)x_res.data_ptr(),
                     (unsigned short*)out.data_ptr(), n, D);
  HIP_CHECK_LAST();
  return out;
}

void adamw_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, long step, double lr, double beta1,
                double beta2, double eps, double wd) {
  check_adamw_flat(p, g, m, v);
  long n = p.numel();
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n)), dim3(BLOCK), 0, stream,
                     p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(), n,
                     (float)beta1, (float)beta2, (float)eps,
                     adam_coef_host(step, lr, beta1, beta2, wd),
                     (const float*)nullptr);
  HIP_CHECK_LAST();
}

// Same update with the coefficients read from ``coef`` (ADAM_NCOEF floats of
// one group, written by adamw_prelude on the same stream).
void adamw_step_dev(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                    torch::Tensor v, torch::Tensor coef, double beta1,
                    double beta2, double eps) {
  check_adamw_flat(p, g, m, v);
  check_adam_coef(coef, p);
  long n = p.numel();
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n)), dim3(BLOCK), 0, stream,
                     p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(), n,
                     (float)beta1, (float)beta2, (float)eps, AdamCoef{},
                     (const float*)coef.data_ptr<float>());
  HIP_CHECK_LAST();
}

// step (int64[1]) += 1; coef[g] = coefficients of group g at the new step
// from hyp[g] = (lr, beta1, beta2, wd) in double.  All three on the device.
void adamw_prelude(torch::Tensor step, torch::Tensor hyp, torch::Tensor coef) {
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == torch::kLong &&
              step.numel() == 1, "adamw_prelude: step must be a device int64");
  TORCH_CHECK(hyp.is_cuda() && hyp.scalar_type() == torch::kDouble &&
              hyp.is_contiguous() && hyp.dim() == 2 &&
              hyp.size(1) == ADAM_NHYP,
              "adamw_prelude: hyp must be a contiguous device double (G, 4)");
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == torch::kFloat &&
              coef.is_contiguous() && coef.dim() == 2 &&
              coef.size(0) == hyp.size(0) && coef.size(1) == ADAM_NCOEF,
              "adamw_prelude: coef must be a contiguous device float (G, 5)");
  TORCH_CHECK(step.get_device() == hyp.get_device() &&
              step.get_device() == coef.get_device());
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(adam_prelude_kernel, dim3(1), dim3(WAVE), 0, stream,
                     (long*)step.data_ptr<int64_t>(), hyp.data_ptr<double>(),
                     coef.data_ptr<float>(), (int)hyp.size(0));
  HIP_CHECK_LAST();
}

namespace {
__global__ void ema_bf16_kernel(float* __restrict__ ema,
                                const unsigned short* __restrict__ p, long n,
                                float decay, float omd, int vec4) {
  // GRID-STRIDED: ew_grid caps launches at 2048 blocks — a plain
  // one-element-per-thread body here updated only the first 524k elements
  // of an 8B-param shard (caught by the large-n parity test); 4-wide
  // vectorized like the fp32 variant (vec4=0: unaligned narrow() views
  // fall back to the scalar loop)
  const long n4 = vec4 ? (n >> 2) : 0;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < n4; i += stride) {
    float4 e = *(const float4*)(ema + i * 4);
    ushort4 v = *(const ushort4*)(p + i * 4);
    e.x = decay * e.x + omd * bf2f(v.x);
    e.y = decay * e.y + omd * bf2f(v.y);
    e.z = decay * e.z + omd * bf2f(v.z);
    e.w = decay * e.w + omd * bf2f(v.w);
    *(float4*)(ema + i * 4) = e;
  }
  for (long i = n4 * 4 + i0; i < n; i += stride)
    ema[i] = decay * ema[i] + omd * bf2f(p[i]);
}
}  // namespace

void ema_update(torch::Tensor ema, torch::Tensor p, double decay) {
  TORCH_CHECK(ema.is_cuda() && ema.scalar_type() == torch::kFloat);
  // both kernels index ema and p 0..ema.numel() as dense arrays
  TORCH_CHECK(p.is_cuda() && p.get_device() == ema.get_device(),
              "ema_update: p must be on ema's device");
  TORCH_CHECK(p.scalar_type() == torch::kFloat ||
              p.scalar_type() == torch::kBFloat16,
              "ema_update: p must be fp32 or bf16");
  TORCH_CHECK(p.numel() == ema.numel(), "ema_update: p has ", p.numel(),
              " elements, ema has ", ema.numel());
  TORCH_CHECK(ema.is_contiguous() && p.is_contiguous(),
              "ema_update: ema and p must be contiguous");
  long n = ema.numel();
  // 1 - decay in double, rounded once: 1.f - 0.9999f is 1.7e-4 off, and an
  // EMA with weights that do not add up to 1 settles that far from p
  const float omd = (float)(1.0 - decay);
  auto stream = at::cuda::getCurrentHIPStream();
  // vector path needs 16B-aligned ema and 16B/8B-aligned p: EMA views are
  // narrow() slices at arbitrary element offsets
  const int vec4 = (((unsigned long long)ema.data_ptr() & 15) == 0 &&
                    ((unsigned long long)p.data_ptr() &
                     (p.scalar_type() == torch::kBFloat16 ? 7 : 15)) == 0)
                   ? 1 : 0;
  if (p.scalar_type() == torch::kBFloat16) {
    // bf16 model params feed the fp32 EMA shard directly — the Python
    // lerp_(p.float()) fallback this replaces materialized an fp32 copy
    // of every param each step (r02 Llama profile: 14% eager elementwise)
    hipLaunchKernelGGL(ema_bf16_kernel, dim3(ew_grid(n, 4)), dim3(BLOCK), 0,
                       stream, ema.data_ptr<float>(),
                       (const unsigned short*)p.data_ptr(), n, (float)decay,
                       omd, vec4);
  } else {
    hipLaunchKernelGGL(ema_kernel, dim3(ew_grid(n, 4)), dim3(BLOCK), 0,
                       stream, ema.data_ptr<float>(), p.data_ptr<float>(), n,
                       (float)decay, omd, vec4);
  }
  HIP_CHECK_LAST();
}

torch::Tensor l2norm_sq(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  auto out = torch::empty({}, x.options().dtype(torch::kFloat));
  long n = x.numel();
  const int grid = ew_grid(n);
  // a single block's partial IS the result; otherwise a second one-block
  // kernel adds the partials in index order
  auto partial = grid == 1 ? out
      : torch::empty({grid}, x.options().dtype(torch::kFloat));
  auto stream = at::cuda::getCurrentHIPStream();
  if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(l2norm_kernel<bf16_t>, dim3(grid), dim3(BLOCK), 0,
                       stream, (const bf16_t*)x.data_ptr(),
                       partial.data_ptr<float>(), n);
  } else {
    hipLaunchKernelGGL(l2norm_kernel<float>, dim3(grid), dim3(BLOCK), 0,
                       stream, x.data_ptr<float>(), partial.data_ptr<float>(),
                       n);
  }
  HIP_CHECK_LAST();
  if (grid > 1) {
    hipLaunchKernelGGL(l2norm_final_kernel, dim3(1), dim3(BLOCK), 0, stream,
                       (const float*)partial.data_ptr<float>(),
                       out.data_ptr<float>(), grid);
    HIP_CHECK_LAST();
  }
  return out;
}

void scale_inplace(torch::Tensor x, double s) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  long n = x.numel();
  auto stream = at::cuda::getCurrentHIPStream();
  if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(scale_kernel<bf16_t>, dim3(ew_grid(n)), dim3(BLOCK), 0,
                       stream, (bf16_t*)x.data_ptr(), n, (float)s);
  } else {
    hipLaunchKernelGGL(scale_kernel<float>, dim3(ew_grid(n)), dim3(BLOCK), 0,
                       stream, x.data_ptr<float>(), n, (float)s);
  }
  HIP_CHECK_LAST();
}

// -------- multi-tensor AdamW: one launch for ALL params ---------------------
// Chunk table built once host-side; per chunk: param id + element offset.
// Reads bf16 grads and writes bf16 params IN the same pass (the v1 profile
// showed the foreach grad-cast + param-copyback pairs costing ~3.6% of step
// on top of the f32 flat update).

namespace {

constexpr long MT_CHUNK = 1 << 16;

__global__ void multi_adamw_kernel(const int* __restrict__ cpid,
                                   const long* __restrict__ coff,
                                   const long* __restrict__ pptrs,
                                   const long* __restrict__ gptrs,
                                   const long* __restrict__ mptrs,
                                   const long* __restrict__ moffs,
                                   const long* __restrict__ numels,
                                   int nchunks,
                                   float* __restrict__ m,
                                   float* __restrict__ v,
                                   float beta1, float beta2, float eps,
                                   AdamCoef ch,
                                   const float* __restrict__ cdev,
                                   int param_bf16, int grad_bf16) {
  const int c = blockIdx.x;
  if (c >= nchunks) return;
  const AdamCoef cf = adam_coef_load(ch, cdev);
  const int pid = cpid[c];
  const long off = coff[c];
  const long n = numels[pid];
  const long end = off + MT_CHUNK < n ? off + MT_CHUNK : n;
  const long mvbase = moffs[pid];     // m/v flat offset
  float* master = (float*)mptrs[pid];  // per-param master (MAY alias param)
  void* pp = (void*)pptrs[pid];
  const void* gp = (const void*)gptrs[pid];
  // grad-None params are SKIPPED entirely (no decay, no moment update) —
  // stock torch.optim semantics; substituting grad=0 silently decayed
  // frozen params toward zero.
  if (gp == nullptr) return;
  // HBM-bound: ~26 B/element of read+write traffic, so dwordx4 accesses are
  // what decides the rate.  All pointers/offsets are 16B-aligned in practice
  // (torch allocations + 64Ki chunking); fall back to scalars otherwise.
  const bool vec4 = ((off | mvbase) & 3) == 0 &&
      (((long)master | (long)pp | (long)gp) & 15) == 0;
  if (vec4) {
    const long nv = (end - off) >> 2;   // full float4 groups in this chunk
    for (long g = threadIdx.x; g < nv; g += blockDim.x) {
      const long i = off + g * 4;
      const long k = mvbase + i;
      float4 gi4;
      if (gp == nullptr) gi4 = make_float4(0.f, 0.f, 0.f, 0.f);
      else if (grad_bf16) {
        ushort4 gu = *(const ushort4*)((const unsigned short*)gp + i);
        gi4 = make_float4(bf2f(gu.x), bf2f(gu.y), bf2f(gu.z), bf2f(gu.w));
      } else {
        gi4 = *(const float4*)((const float*)gp + i);
      }
      float4 p4 = *(const float4*)(master + i);
      float4 m4 = *(const float4*)(m + k);
      float4 v4 = *(const float4*)(v + k);
      float* pi = (float*)&p4;
      float* mi = (float*)&m4;
      float* vi = (float*)&v4;
      const float* gi = (const float*)&gi4;
      ushort4 pb;
      unsigned short* pbs = (unsigned short*)&pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        adam_elem(pi[j], mi[j], vi[j], gi[j], beta1, beta2, eps, cf);
        pbs[j] = f2bf(pi[j]);
      }
      *(float4*)(m + k) = m4;
      *(float4*)(v + k) = v4;
      *(float4*)(master + i) = p4;
      if (param_bf16) *(ushort4*)((unsigned short*)pp + i) = pb;
    }
    // scalar tail: at most 3 elements at the chunk end
    for (long i = off + nv * 4 + threadIdx.x; i < end; i += blockDim.x) {
      float gi;
      if (gp == nullptr) gi = 0.f;
      else if (grad_bf16) gi = bf2f(((const unsigned short*)gp)[i]);
      else gi = ((const float*)gp)[i];
      const long k = mvbase + i;
      float pi = master[i], mi = m[k], vi = v[k];
      adam_elem(pi, mi, vi, gi, beta1, beta2, eps, cf);
      m[k] = mi;
      v[k] = vi;
      master[i] = pi;
      if (param_bf16) ((unsigned short*)pp)[i] = f2bf(pi);
    }
    return;
  }
  for (long i = off + threadIdx.x; i < end; i += blockDim.x) {
    float gi;
    if (gp == nullptr) gi = 0.f;
    else if (grad_bf16) gi = bf2f(((const unsigned short*)gp)[i]);
    else gi = ((const float*)gp)[i];
    const long k = mvbase + i;
    float pi = master[i], mi = m[k], vi = v[k];
    adam_elem(pi, mi, vi, gi, beta1, beta2, eps, cf);
    m[k] = mi;
    v[k] = vi;
    master[i] = pi;
    if (param_bf16) ((unsigned short*)pp)[i] = f2bf(pi);
  }
}

}  // namespace

namespace {
void launch_multi_adamw(const torch::Tensor& cpid, const torch::Tensor& coff,
                        const torch::Tensor& pptrs, const torch::Tensor& gptrs,
                        const torch::Tensor& mptrs, const torch::Tensor& moffs,
                        const torch::Tensor& numels, const torch::Tensor& m,
                        const torch::Tensor& v, double beta1, double beta2,
                        double eps, AdamCoef ch, const float* cdev,
                        bool param_bf16, bool grad_bf16) {
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == torch::kFloat);
  int nchunks = cpid.numel();
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(multi_adamw_kernel, dim3(nchunks), dim3(BLOCK), 0,
                     stream, cpid.data_ptr<int>(), coff.data_ptr<long>(),
                     pptrs.data_ptr<long>(), gptrs.data_ptr<long>(),
                     mptrs.data_ptr<long>(), moffs.data_ptr<long>(),
                     numels.data_ptr<long>(),
                     nchunks, m.data_ptr<float>(),
                     v.data_ptr<float>(), (float)beta1, (float)beta2,
                     (float)eps, ch, cdev,
                     param_bf16 ? 1 : 0, grad_bf16 ? 1 : 0);
  HIP_CHECK_LAST();
}
}  // namespace

void multi_adamw_step(torch::Tensor cpid, torch::Tensor coff,
                      torch::Tensor pptrs, torch::Tensor gptrs,
                      torch::Tensor mptrs, torch::Tensor moffs,
                      torch::Tensor numels,
                      torch::Tensor m, torch::Tensor v,
                      long step, double lr, double beta1, double beta2,
                      double eps, double wd, bool param_bf16,
                      bool grad_bf16) {
  launch_multi_adamw(cpid, coff, pptrs, gptrs, mptrs, moffs, numels, m, v,
                     beta1, beta2, eps,
                     adam_coef_host(step, lr, beta1, beta2, wd), nullptr,
                     param_bf16, grad_bf16);
}

// The capturable form: coefficients of this group from device memory
// (written by adamw_prelude on the same stream).
void multi_adamw_step_dev(torch::Tensor cpid, torch::Tensor coff,
                          torch::Tensor pptrs, torch::Tensor gptrs,
                          torch::Tensor mptrs, torch::Tensor moffs,
                          torch::Tensor numels,
                          torch::Tensor m, torch::Tensor v,
                          torch::Tensor coef, double beta1, double beta2,
                          double eps, bool param_bf16, bool grad_bf16) {
  check_adam_coef(coef, m);
  launch_multi_adamw(cpid, coff, pptrs, gptrs, mptrs, moffs, numels, m, v,
                     beta1, beta2, eps, AdamCoef{}, coef.data_ptr<float>(),
                     param_bf16, grad_bf16);
}
