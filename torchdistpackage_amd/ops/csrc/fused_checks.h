// Operand checks shared by the fused residual-stream bindings in norms.hip
// and elementwise.hip.  Their kernels index every operand as a dense bf16
// array of the reference tensor's shape with 16-byte (or 8-byte pair) vector
// accesses and check nothing themselves, so everything is checked here,
// before any launch.
#pragma once

#include <torch/extension.h>

// 16 bytes is what torch allocations and every row offset (D % 8 == 0) give
inline bool aligned16(const torch::Tensor& t) {
  return ((unsigned long long)t.data_ptr() & 15) == 0;
}

// t: bf16, contiguous, aligned, on like's device, of like's shape
inline void check_bf16_rows(const char* fn, const char* name,
                            const torch::Tensor& t,
                            const torch::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == torch::kBFloat16 && t.is_contiguous() &&
                  t.sizes() == like.sizes() && aligned16(t),
              fn, ": ", name,
              " must be a contiguous, 16-byte aligned bf16 tensor of shape ",
              like.sizes(), " on ", like.device(), ", got ", t.scalar_type(),
              " ", t.sizes(), " on ", t.device());
}

// t: bf16, contiguous, aligned, on like's device, D elements
inline void check_bf16_vec(const char* fn, const char* name,
                           const torch::Tensor& t, const torch::Tensor& like,
                           int D) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == torch::kBFloat16 && t.is_contiguous() &&
                  t.numel() == D && aligned16(t),
              fn, ": ", name,
              " must be a contiguous, 16-byte aligned bf16 vector of ", D,
              " elements on ", like.device());
}
