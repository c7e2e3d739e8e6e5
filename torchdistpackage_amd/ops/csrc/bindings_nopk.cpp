// pybind11 bindings of the _tdpa_nopk module: the translation units that
// ops/build.py compiles without packed-fp32 VALU forms.
#include <torch/extension.h>

torch::Tensor decode_attention_paged(torch::Tensor q, torch::Tensor k_pool,
                                     torch::Tensor v_pool,
                                     torch::Tensor block_table,
                                     torch::Tensor out,
                                     c10::optional<torch::Tensor> pos_t,
                                     long pos0, double scale, long split_kv);
void kv_paged_append(torch::Tensor k_pool, torch::Tensor v_pool,
                     torch::Tensor block_table, torch::Tensor k,
                     torch::Tensor v, c10::optional<torch::Tensor> pos_t,
                     long pos0);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("decode_attention_paged", &decode_attention_paged,
        "(q, k_pool, v_pool, block_table, out, pos_t|None, pos0, scale, "
        "split_kv) -> out");
  m.def("kv_paged_append", &kv_paged_append,
        "(k_pool, v_pool, block_table, k, v, pos_t|None, pos0)");
}
