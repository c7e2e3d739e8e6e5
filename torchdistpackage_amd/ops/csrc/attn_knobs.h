// Run-time switches of the training attention dispatch (attention.hip,
// attention_v2.hip).  Initialised once from the environment; the bindings
// attn_knobs() / attn_set_knobs() read and replace them (docs/knobs.md).
#pragma once

#include <cstdint>

struct AttnKnobs {
  bool dq_recompute;     // TDPA_DQ_RECOMPUTE: no-workspace backward
  bool no_tr16;          // TDPA_NO_TR16: no hardware transpose reads in the
                         // backward: two-pass dk/dv and the scatter dq-lite
  bool pstore;           // TDPA_PSTORE: dv pass stores P for the dk pass
  bool force_v1;         // TDPA_ATTN_V1: head dim 128 through the v1 kernels
  int64_t max_ds_bytes;  // dS (+P) workspace cap; above it: recompute route
  bool split_dkdv;       // TDPA_SPLIT_DKDV: two-pass dk/dv on every v2 route
};

AttnKnobs& attn_knobs_ref();   // attention.hip

// What attn_bwd launches.  v1: the pair in attention.hip; otherwise the v2
// kernels, either the no-workspace recompute route or the dS-workspace route
// with its two options.  attn_bwd dispatches on this struct and
// attn_bwd_route() names it, so the name cannot drift from the launch.
// dk and dv come from the fused kernel unless two_pass(); split_dkdv is set
// only where that knob alone selects the two passes.
struct AttnBwdRoute {
  bool v1, recompute, pstore, no_tr16, split_dkdv;
  bool two_pass() const { return pstore || no_tr16 || split_dkdv; }
};

AttnBwdRoute attn_bwd_select(const AttnKnobs& knobs, int64_t B, int64_t H,
                             int64_t S, int64_t D);   // attention_v2.hip

// dv = P^T @ dO runs on the bf16 MFMA, whose adder aligns the products and
// the accumulator to the largest of them and floors whatever falls below that
// window: a product of -1e-19 next to a +-4 comes out as -2^-22, 10^12 times
// its value, and survives when the large terms cancel (torch's own bf16 GEMM
// does the same).  The dv passes therefore feed the MFMA an exact 0 for any
// P below this.  What is dropped is below 2^-40 of the key's attended terms;
// a key that no row attends to above 2^-40 gets dv = 0 exactly where it had
// about 1e-13 * do.  dS, dq and dk keep the full P, except under pstore,
// whose dk pass rebuilds dS from the P the dv pass stored, flush included.
// In the v2 dv pass the test is folded into the validity mask's select (one
// compare per element).
constexpr float kAttnPFlush = 0x1p-40f;
