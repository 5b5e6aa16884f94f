// Launch helpers shared by nn.hip and the once-compiled files split from it (nn_resize_eval.hip, nn_float_ops.hip):
// the workgroup size, the capped grid of a grid-stride launch and the stream cast.  PRIVATE to csrc/.
#pragma once
#include "dspn_common.h"

namespace {

constexpr int kT = 256;

inline int grid_for(long long n, int per_block = kT, int cap = 8192) {
  long long b = (n + per_block - 1) / per_block;
  return (int)std::max<long long>(1, std::min<long long>(b, cap));
}

}  // namespace

#define S_(x) ((hipStream_t)(x))
