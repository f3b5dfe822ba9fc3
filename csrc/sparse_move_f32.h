// The fp32 table's gather, assign and add launchers (kernels.hip), the fp32
// branch of kernels.h's SparseGather, SparseScatterAssign and
// SparseScatterAdd in sparse_table.hip. Internal to those two files.
#pragma once

#include "kernels.h"

namespace xps {
namespace kern {

void SparseGatherF32(const float* table, const SparseRows& rows, float* out);
void SparseScatterAssignF32(float* table, const SparseRows& rows, const float* src);
void SparseScatterAddF32(float* table, const SparseRows& rows, const float* src, bool atomic);

}  // namespace kern
}  // namespace xps
