// Python bindings for the in-tree gfx950 HIP extension (_tdpa_hip).
#include <torch/extension.h>

#include "grouped_gemm_plan.h"

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps);
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor rstd);
std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps);
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd);
torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias);
torch::Tensor bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                            torch::Tensor bias);
void adamw_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, long step, double lr, double beta1,
                double beta2, double eps, double wd);
void multi_adamw_step(torch::Tensor cpid, torch::Tensor coff,
                      torch::Tensor pptrs, torch::Tensor gptrs,
                      torch::Tensor mptrs, torch::Tensor moffs,
                      torch::Tensor numels,
                      torch::Tensor m, torch::Tensor v,
                      long step, double lr, double beta1, double beta2,
                      double eps, double wd, bool param_bf16, bool grad_bf16);
void adamw_step_dev(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                    torch::Tensor v, torch::Tensor coef, double beta1,
                    double beta2, double eps);
void adamw_prelude(torch::Tensor step, torch::Tensor hyp, torch::Tensor coef);
void multi_adamw_step_dev(torch::Tensor cpid, torch::Tensor coff,
                          torch::Tensor pptrs, torch::Tensor gptrs,
                          torch::Tensor mptrs, torch::Tensor moffs,
                          torch::Tensor numels,
                          torch::Tensor m, torch::Tensor v,
                          torch::Tensor coef, double beta1, double beta2,
                          double eps, bool param_bf16, bool grad_bf16);
void ema_update(torch::Tensor ema, torch::Tensor p, double decay);
torch::Tensor l2norm_sq(torch::Tensor x);
void scale_inplace(torch::Tensor x, double s);
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o,
                                    bool causal, double scale);
std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    torch::Tensor dq, torch::Tensor dk,
                                    torch::Tensor dv,
                                    bool causal, double scale);
std::tuple<bool, bool, bool, bool, int64_t, bool> attn_knobs();
std::tuple<bool, bool, bool, bool, int64_t, bool> attn_set_knobs(
    bool dq_recompute, bool no_tr16, bool pstore, bool force_v1,
    int64_t max_ds_bytes, bool split_dkdv);
std::string attn_bwd_route(int64_t B, int64_t H, int64_t S, int64_t D);
torch::Tensor mfma_probe_16x16x32(torch::Tensor a, torch::Tensor b);
torch::Tensor mfma_probe_32x32x16(torch::Tensor a, torch::Tensor b);
torch::Tensor tr16_probe(long addr_mode);
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor targets);
torch::Tensor gemm_fprop(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias);
torch::Tensor rope_apply(torch::Tensor x, torch::Tensor cs, torch::Tensor sn,
                         long pos0, bool fwd);
torch::Tensor swiglu_fwd(torch::Tensor a, torch::Tensor b);
torch::Tensor bgelu_b_fwd(torch::Tensor x, torch::Tensor bias);
torch::Tensor bgelu_b_bwd(torch::Tensor dy, torch::Tensor x,
                          torch::Tensor bias);
std::vector<torch::Tensor> swiglu_bwd(torch::Tensor dy, torch::Tensor a,
                                      torch::Tensor b);
torch::Tensor gemm_dgrad(torch::Tensor dy, torch::Tensor w, bool kswz);
torch::Tensor gemm_wgrad(torch::Tensor dy, torch::Tensor x, long splitk,
                         bool kswz);
torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets,
                     torch::Tensor lse, torch::Tensor grad_out);
std::vector<torch::Tensor> ce_partial_fwd(torch::Tensor logits,
                                          torch::Tensor targets);
torch::Tensor gemv_bf16(torch::Tensor x, torch::Tensor W,
                        c10::optional<torch::Tensor> bias);
torch::Tensor gemv_w8a16(torch::Tensor x, torch::Tensor q,
                         torch::Tensor scale,
                         c10::optional<torch::Tensor> bias);
torch::Tensor rope_apply_pos(torch::Tensor x, torch::Tensor cs,
                             torch::Tensor sn, torch::Tensor pos, bool fwd);
torch::Tensor decode_attention(torch::Tensor q, torch::Tensor k_cache,
                               torch::Tensor v_cache, torch::Tensor out,
                               c10::optional<torch::Tensor> pos_t, long pos0,
                               double scale, long split_kv);
torch::Tensor grouped_gemm_fprop(torch::Tensor x, torch::Tensor w,
                                 torch::Tensor offs,
                                 c10::optional<torch::Tensor> bias);
torch::Tensor grouped_gemm_dgrad(torch::Tensor dy, torch::Tensor w,
                                 torch::Tensor offs);
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> grouped_gemm_wgrad(
    torch::Tensor dy, torch::Tensor x, torch::Tensor offs,
    bool want_bias_grad);
torch::Tensor grouped_gemm_plan(torch::Tensor offs_cpu, int64_t T);
std::vector<torch::Tensor> bias_residual_layernorm_fwd(
    torch::Tensor y, c10::optional<torch::Tensor> bias, torch::Tensor x_res,
    torch::Tensor ln_w, torch::Tensor ln_b, double eps);
std::vector<torch::Tensor> layernorm_bwd_residual(
    torch::Tensor dh, torch::Tensor x, torch::Tensor w, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor g_res, bool want_colsum);
std::vector<torch::Tensor> bias_gelu_bwd_colsum(torch::Tensor dy,
                                                torch::Tensor x,
                                                torch::Tensor bias);
bool bias_gelu_bwd_colsum_ok(int64_t D);
int64_t fused_ln_max_d();
torch::Tensor bias_residual_add(torch::Tensor y,
                                c10::optional<torch::Tensor> bias,
                                torch::Tensor x_res);
torch::Tensor attn_delta(torch::Tensor o, torch::Tensor dout);
void attn_bwd_dkdv(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                   torch::Tensor v, torch::Tensor lse, torch::Tensor delta,
                   torch::Tensor dk, torch::Tensor dv, bool causal,
                   double scale);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("adamw_step", &adamw_step);
  m.def("multi_adamw_step", &multi_adamw_step);
  m.def("adamw_step_dev", &adamw_step_dev);
  m.def("adamw_prelude", &adamw_prelude);
  m.def("multi_adamw_step_dev", &multi_adamw_step_dev);
  m.def("ema_update", &ema_update);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("scale_inplace", &scale_inplace);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_knobs", &attn_knobs,
        "(dq_recompute, no_tr16, pstore, force_v1, max_ds_bytes, split_dkdv)");
  m.def("attn_set_knobs", &attn_set_knobs,
        "set the six attention knobs; returns the previous six");
  m.def("attn_bwd_route", &attn_bwd_route,
        "name of the backward route for (B, H, S, D) under the current knobs");
  m.def("mfma_probe_16x16x32", &mfma_probe_16x16x32);
  m.def("mfma_probe_32x32x16", &mfma_probe_32x32x16);
  m.def("tr16_probe", &tr16_probe);
  m.def("ce_fwd", &ce_fwd);
  m.def("gemm_fprop", &gemm_fprop);
  m.def("rope_apply", &rope_apply);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("bgelu_b_fwd", &bgelu_b_fwd);
  m.def("bgelu_b_bwd", &bgelu_b_bwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("gemm_dgrad", &gemm_dgrad);
  m.def("gemm_wgrad", &gemm_wgrad);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_partial_fwd", &ce_partial_fwd);
  m.def("gemv_bf16", &gemv_bf16);
  m.def("gemv_w8a16", &gemv_w8a16);
  m.def("rope_apply_pos", &rope_apply_pos);
  m.def("decode_attention", &decode_attention);
  m.def("grouped_gemm_fprop", &grouped_gemm_fprop);
  m.def("grouped_gemm_dgrad", &grouped_gemm_dgrad);
  m.def("grouped_gemm_wgrad", &grouped_gemm_wgrad);
  m.def("grouped_gemm_plan", &grouped_gemm_plan,
        "(offs_cpu, T) -> (row-tile bound, 3) int64: (expert, first row, "
        "row count) per block, expert -1 = idle");
  m.attr("GROUPED_GEMM_BM") = GG_BM;
  m.def("bias_residual_layernorm_fwd", &bias_residual_layernorm_fwd,
        "(y, bias|None, x_res, ln_w, ln_b, eps) -> (x_new, h, mean, rstd)");
  m.def("layernorm_bwd_residual", &layernorm_bwd_residual,
        "(dh, x, w, mean, rstd, g_res, want_colsum) -> (g, partial): "
        "fp32 (2|3, grid, D); partial[k].sum(0), one sum per slice, = dw, db"
        "[, colsum(g)] (one sum(1) would change the bits of dw and db)");
  m.def("bias_gelu_bwd_colsum", &bias_gelu_bwd_colsum,
        "(dy, x, bias) -> (dx, partial): partial.sum(0) = colsum(dx) in fp32");
  m.def("fused_ln_max_d", &fused_ln_max_d,
        "widest last dim of the fused LayerNorm kernels");
  m.def("bias_gelu_bwd_colsum_ok", &bias_gelu_bwd_colsum_ok,
        "whether bias_gelu_bwd_colsum covers last dim D");
  m.def("bias_residual_add", &bias_residual_add,
        "(y, bias|None, x_res) -> bf16(x_res + bf16(y + bias))");
  m.def("attn_delta", &attn_delta,
        "(o, dout) (B, H, S, D) bf16 -> rowsum(o * dout) (B, H, S) fp32");
  m.def("attn_bwd_dkdv", &attn_bwd_dkdv,
        "(dout, q, k, v, lse, delta, dk, dv, causal, scale): the dk/dv stage "
        "of the head-dim-128 backward alone, under the current knobs");
}
