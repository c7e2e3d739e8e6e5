// Limits of the MoE routing kernels (csrc/moe_route.hip), shared with the
// bindings, which export MOE_PLAN_CHUNK to Python.
#pragma once

// routing entries one workgroup of the plan kernels covers; N*k at or below
// it takes the single-launch plan
constexpr int MOE_PLAN_CHUNK = 2048;
constexpr int MOE_ROUTE_MAX_E = 256;   // experts (one LDS histogram column each)
constexpr int MOE_ROUTE_MAX_K = 8;     // routing slots per token
