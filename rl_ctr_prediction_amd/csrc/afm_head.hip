// AFM's out head (p_model.AFM.forward, reference src/models/p_model.py:483-486) for the fused
// training step: everything between the attention pooling and its backward, in one launch.
//
// Per example b:  z_lr = bias + sum_f lin[x_bf]  (ctr_lr_forward's order: the F weights added
// in field order, then the bias);  z = z_lr + (<pooled_b, fc_w> + fc_b)  (ctr_deepfm_head's dot:
// head_lane_dot per lane of a 64-lane row, then the xor butterfly 32 .. 1);  the BCE head of
// ctr_common.h;  dpooled[b, k] = gz[b] * fc_w[k].
//
// B * (F + K) floats come in: the kernel is bound by the latency of its dependent loads (id ->
// weight, then the reduction), not by bytes, so a wave holds 64 / G rows, G = the power of two
// >= F, at least 16 (the driver's F = 15: four rows a wave). A row's G lanes gather one linear
// weight each; the 64 lane values of the head's dot are dealt over them, lane g holding the
// values g, g + G, ...: the butterfly's steps 32 .. G are adds between a lane's own registers
// (the same pairs), its steps G/2 .. 1 shuffles inside the row's lane group. Every lane of a row
// ends with the row's z, p, loss and gz; lane 0 writes them, all of them write dpooled from the
// fc_w values the dot already holds. A row's results depend on the row alone.
#include "ctr_common.h"
#include "head_dot.h"

namespace ctr {

constexpr int kAfmHeadMaxF = 64;
constexpr int kAfmHeadMaxK = 128;
constexpr int kAfmHeadJ = kAfmHeadMaxK / kWave;  // columns of a dot lane

template <typename IdxT, int G>
__global__ __launch_bounds__(256) void afm_head_kernel(
    const IdxT* __restrict__ idx, int64_t B, int F, int K, int64_t V,
    const float* __restrict__ lin, const float* __restrict__ bias,
    const float* __restrict__ pooled, int64_t ldp, const float* __restrict__ fc_w,
    const float* __restrict__ fc_b, const float* __restrict__ labels, float mean_div,
    float* __restrict__ z_out, float* __restrict__ p_out, float* __restrict__ loss_out,
    float* __restrict__ gz_out, float* __restrict__ dpooled, int64_t ldg, int32_t* err) {
  constexpr int R = kWave / G;  // rows of a wave = dot lanes of a lane
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (wave * R >= B) return;  // wave-uniform
  const int g = lane % G, base = lane - g;
  const int64_t b = wave * R + lane / G;
  const bool row = b < B;
  const float yb = row ? labels[b] : 0.f;  // in flight with the gathers
  float wl = 0.f;
  if (row && g < F) wl = lin[load_row(idx, b * F + g, V, err)];
  // the head's dot: this lane's R of the row's 64 lane values (none for a row past the batch)
  const float* hb = pooled + (row ? b : 0) * ldp;
  float hv[R][kAfmHeadJ], wv[R][kAfmHeadJ], val[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    val[r] = head_lane_dot<kAfmHeadJ>(hb, fc_w, row ? K : 0, g + G * r, hv[r], wv[r]);
#pragma unroll
  for (int m = R / 2; m > 0; m >>= 1) {  // the butterfly's steps 32 .. G
#pragma unroll
    for (int r = 0; r < m; ++r) val[r] = val[r] + val[r + m];
  }
  float dot = val[0];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, kWave);  // steps G/2 .. 1
  // the linear term, in field order (F <= G; every lane takes part in the broadcasts)
  float acc = 0.f;
  for (int j = 0; j < F; ++j) {
    const float v = __shfl(wl, base + j, kWave);
    acc = j == 0 ? v : acc + v;
  }
  const float z_lr = bias[0] + acc;              // ctr_lr_forward
  const float z = z_lr + (dot + fc_b[0]);        // ctr_deepfm_head
  float p, l, gz;
  bce_sigmoid_head(z, yb, mean_div, p, l, gz);
  if (!row) return;
  if (g == 0) {
    if (z_out) z_out[b] = z;
    if (p_out) p_out[b] = p;
    if (loss_out) loss_out[b] = l;
    gz_out[b] = gz;
  }
  float* d = dpooled + b * ldg;
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int q = 0; q < kAfmHeadJ; ++q) {
      const int j = g + G * r + q * kWave;
      if (j < K) d[j] = gz * wv[r][q];
    }
  }
}

}  // namespace ctr

using namespace ctr;

extern "C" int ctr_afm_head(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                            const float* lin, const float* bias, const float* pooled,
                            int64_t ldp, const float* fc_w, const float* fc_b,
                            const float* labels, float mean_div, float* z, float* p,
                            float* loss_elem, float* gz, float* dpooled, int64_t ldg,
                            int32_t* err_flag, ctr_stream_t stream) {
  CTR_REQUIRE(B >= 0 && V >= 1, "ctr_afm_head: bad sizes B=%lld V=%lld", (long long)B,
              (long long)V);
  CTR_REQUIRE(F >= 2 && F <= kAfmHeadMaxF, "ctr_afm_head: F=%d outside [2, %d]", F, kAfmHeadMaxF);
  CTR_REQUIRE(K >= 1 && K <= kAfmHeadMaxK, "ctr_afm_head: K=%d outside [1, %d]", K, kAfmHeadMaxK);
  CTR_REQUIRE(idx_type == CTR_IDX_I32 || idx_type == CTR_IDX_I64, "ctr_afm_head: bad idx_type %d",
              idx_type);
  CTR_REQUIRE(lin && bias && fc_w && fc_b, "ctr_afm_head: null lin / bias / fc_w / fc_b");
  CTR_REQUIRE((idx && pooled && labels && gz && dpooled) || B == 0,
              "ctr_afm_head: null idx / pooled / labels / gz / dpooled");
  CTR_REQUIRE(ldp >= K && ldg >= K, "ctr_afm_head: ldp %lld or ldg %lld < K = %d", (long long)ldp,
              (long long)ldg, K);
  CTR_REQUIRE(mean_div > 0.f, "ctr_afm_head: mean_div must be > 0");
  if (B == 0) return CTR_OK;
  int G = 16;
  while (G < F) G <<= 1;
  const int64_t waves = ceil_div(B, kWave / G);
  hipStream_t st = as_stream(stream);
  dispatch_width(G, [&](auto gw) {  // 16, 32 or 64
    constexpr int GW = decltype(gw)::value < 16 ? 16 : decltype(gw)::value;
    dispatch_bool(idx_type == CTR_IDX_I64, [&](auto i64) {
      using IdxT = std::conditional_t<decltype(i64)::value, int64_t, int32_t>;
      hipLaunchKernelGGL((afm_head_kernel<IdxT, GW>), (unsigned)ceil_div(waves, 4), 256, 0, st,
                         static_cast<const IdxT*>(idx), B, F, K, V, lin, bias, pooled, ldp, fc_w,
                         fc_b, labels, mean_div, z, p, loss_elem, gz, dpooled, ldg, err_flag);
    });
  });
  CTR_LAUNCH_CHECK("ctr_afm_head");
  return CTR_OK;
}
