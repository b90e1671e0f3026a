// The Linear(H, 1) dot of the out heads (ctr_deepfm_head, ctr_afm_head): one place holds its
// term order, so the heads agree bit for bit.
#pragma once

#include "ctr_common.h"

namespace ctr {

// Lane `lane` (0..63) of a row's dot over H <= MAXJ * 64 columns: the lane's columns lane,
// lane + 64, ... are loaded together (and kept in hv / wv for the caller's gradient), their
// products added in that order. The row's dot is the xor butterfly 32, 16, ..., 1 over the 64
// lane values (wave_sum, or the same tree over registers where a lane holds several of them).
template <int MAXJ>
__device__ __forceinline__ float head_lane_dot(const float* hb, const float* w, int H, int lane,
                                               float (&hv)[MAXJ], float (&wv)[MAXJ]) {
  float part = 0.f;
#pragma unroll
  for (int q = 0; q < MAXJ; ++q) {
    const int j = lane + q * kWave;
    hv[q] = j < H ? hb[j] : 0.f;
    wv[q] = j < H ? w[j] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < MAXJ; ++q)
    if (lane + q * kWave < H) part += hv[q] * wv[q];
  return part;
}

}  // namespace ctr
