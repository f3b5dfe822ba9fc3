// The per-element arithmetic of the sparse optimizer steps (sparse_table.hip),
// stated once for every table and wire and compiled with unpaired fp32
// operations, so a step computes the same fp32 value whatever the table
// stores.
#pragma once

#include <hip/hip_runtime.h>

namespace xps {
namespace kern {

// Adagrad. IEEE multiply, square root, add, divide and subtract, in that
// order: the tests' error bound counts one rounding for each
__device__ inline float Step(float w, float g, float lr, float denom) {
  return w - (lr * g) / denom;
}
__device__ inline float Denom(float s, float eps) { return sqrtf(s) + eps; }

// Lazy Adam. beta * old + omb * x: both moments, the row-wise second one
// included. Two rounded products and their rounded sum: left to the compiler,
// either product may be fused into the add, and two kernels have chosen
// differently (a last-bit difference in m' and v'), so contraction is off here
__device__ inline float Moment(float old, float x, float beta, float omb) {
#pragma clang fp contract(off)
  return beta * old + omb * x;
}
__device__ inline float AdamDenom(float v, float c2, float eps) { return sqrtf(v / c2) + eps; }
__device__ inline float AdamStep(float w, float m, float alpha, float denom) {
  return w - (alpha * m) / denom;
}

// a lazy-Adam record's header {p1, p2, v_row, 0}: one 16 B access on the
// vector paths (state base and record length are multiples of 16 B there),
// four floats on the scalar paths
template <bool kVec>
__device__ inline float4 LoadHeader(const float* rec) {
  if (kVec) return *reinterpret_cast<const float4*>(rec);
  return float4{rec[0], rec[1], rec[2], rec[3]};
}
template <bool kVec>
__device__ inline void StoreHeader(float* rec, float4 h) {
  if (kVec) {
    *reinterpret_cast<float4*>(rec) = h;
  } else {
    rec[0] = h.x;
    rec[1] = h.y;
    rec[2] = h.z;
    rec[3] = h.w;
  }
}

}  // namespace kern
}  // namespace xps
