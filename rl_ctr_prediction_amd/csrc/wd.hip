// Wide&Deep (W&D): the MLP input and the wide logit of p_model.WideAndDeep (reference
// src/models/p_model.py:103-144),
//   p = sigmoid((bias + sum_f lin[x_f]) + mlp(flat(embedding[x])))
// — DeepFM without the second-order term. One launch gathers embedding[x] and writes it as
// the MLP input (the three bf16 operand planes of gemm_planes.hip and / or the fp32 [B, F*K]
// matrix) and writes z_lin[b] = bias[0] + sum_f lin[x_bf]. No field sum, no square sums:
// nothing of size B*K besides the input itself.
//
// The kernel is a bandwidth-bound stream laid out like csrc/opnn.hip's forward: one thread
// owns one 16-byte column piece (K % 4 == 0 and every pointer / stride 16-byte aligned) or
// one column (any K, e.g. the drivers' latent_dims = 10) of one example and walks the F
// fields with kWdInFlight row loads in flight; the K/4 (or K) threads of an example read and
// write each row as one contiguous run. The block's threads resolve the ids of the block's
// examples (one contiguous run of idx) once, in parallel, into LDS, and gather the linear
// weight of every id beside it, so the F weight gathers of an example are F independent
// loads of different threads. The thread that owns an example's first piece then adds the
// example's F weights in field order and the bias last: a row's z_lin (and its input) are
// the same bits at any B and any position in the batch. Blocks whose ids do not fit
// kWdStageBytes of LDS (K of a few columns with hundreds of fields) walk their ids
// themselves, with the same additions in the same order.
#include "ctr_common.h"

namespace ctr {

constexpr int kWdInFlight = 8;
constexpr int kWdBlock = 256;
constexpr size_t kWdStageBytes = 32 * 1024;  // LDS for a block's resolved ids + weights
constexpr size_t kWdStageEntry = sizeof(long long) + sizeof(float);

template <int VEC>
struct wd_vec;
template <>
struct wd_vec<1> {
  typedef float type;
};
template <>
struct wd_vec<4> {
  typedef float4 type;
};

__device__ __forceinline__ float wd_zero(float) { return 0.f; }
__device__ __forceinline__ float4 wd_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

// the three bf16 planes of one element / of four consecutive elements at row base xb + col
__device__ __forceinline__ void wd_store_planes(uint16_t* xb, int64_t ps, float v) {
  uint16_t h3[3];
  psplit1(v, h3);
#pragma unroll
  for (int q = 0; q < 3; ++q) xb[q * ps] = h3[q];
}
__device__ __forceinline__ void wd_store_planes(uint16_t* xb, int64_t ps, float4 v) {
  store_planes4_at(xb, ps, v);
}

// piece g of the B * KV pieces -> its example; small: B * KV < 2^32 (one 32-bit division)
__device__ __forceinline__ int64_t wd_example(int64_t g, int KV, bool small) {
  return small ? (int64_t)((uint32_t)g / (uint32_t)KV) : g / KV;
}

// stage_n: the LDS holds stage_n ids (long long) followed by stage_n weights (float)
template <typename IdxT, int VEC, bool STAGE>
__global__ __launch_bounds__(kWdBlock) void wd_forward_kernel(
    const IdxT* __restrict__ idx, int64_t B, int F, int K, int64_t V,
    const float* __restrict__ emb, const float* __restrict__ lin,
    const float* __restrict__ bias, float* __restrict__ flat, int64_t ldf,
    uint16_t* __restrict__ xpl, int64_t xpl_ld, int64_t xpl_ps, float* __restrict__ z_lin,
    int stage_n, int32_t* err) {
  typedef typename wd_vec<VEC>::type VT;
  extern __shared__ __attribute__((aligned(16))) long long wd_staged_rows[];
  float* staged_lin = reinterpret_cast<float*>(wd_staged_rows + stage_n);
  const int KV = K / VEC;
  const int64_t n = B * KV;
  const bool small = (n >> 32) == 0;
  int64_t b0 = 0;
  if (STAGE) {  // the rows of the block's examples b0 .. b1: ids idx[b0*F, (b1+1)*F)
    const int64_t g0 = (int64_t)blockIdx.x * blockDim.x;  // < n: the grid covers n pieces
    const int64_t g1 = (g0 + blockDim.x < n ? g0 + blockDim.x : n) - 1;
    b0 = wd_example(g0, KV, small);
    const int64_t nid = (wd_example(g1, KV, small) - b0 + 1) * F;  // host: <= stage_n
    for (int64_t i = threadIdx.x; i < nid; i += blockDim.x) {
      const int64_t r = load_row(idx, b0 * F + i, V, err);
      wd_staged_rows[i] = (long long)r;
      staged_lin[i] = lin[r];
    }
    __syncthreads();
  }
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;  // after the block's only barrier
  const int64_t b = wd_example(gid, KV, small);
  const int k = (int)(gid - b * KV) * VEC;
  float* ob = flat ? flat + b * ldf + k : nullptr;
  uint16_t* xb = xpl ? xpl + b * xpl_ld + k : nullptr;
  const IdxT* ids = idx + b * F;
  const long long* my_rows = wd_staged_rows + (b - b0) * F;
  for (int f0 = 0; f0 < F; f0 += kWdInFlight) {
    int64_t row[kWdInFlight];
    VT v[kWdInFlight];
#pragma unroll
    for (int u = 0; u < kWdInFlight; ++u)
      row[u] = f0 + u >= F ? 0
               : STAGE ? (int64_t)my_rows[f0 + u]
                       : load_row(ids, (int64_t)(f0 + u), V, err);
#pragma unroll
    for (int u = 0; u < kWdInFlight; ++u)
      v[u] = f0 + u < F ? *reinterpret_cast<const VT*>(emb + row[u] * K + k) : wd_zero(VT());
#pragma unroll
    for (int u = 0; u < kWdInFlight; ++u) {
      if (f0 + u < F) {  // block-uniform
        const int64_t col = (int64_t)(f0 + u) * K;
        if (ob) *reinterpret_cast<VT*>(ob + col) = v[u];
        if (xb) wd_store_planes(xb + col, xpl_ps, v[u]);
      }
    }
  }
  if (k == 0) {  // the example's first piece: lin[x_0] + lin[x_1] + ... in field order, + bias
    const float* my_lin = staged_lin + (b - b0) * F;
    float acc = 0.f;
    for (int f = 0; f < F; ++f) {
      const float w = STAGE ? my_lin[f] : lin[load_row(ids, (int64_t)f, V, nullptr)];
      acc = f == 0 ? w : acc + w;
    }
    z_lin[b] = bias[0] + acc;  // p_model.py:142
  }
}

}  // namespace ctr

using namespace ctr;

static bool wd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int ctr_wd_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                              const float* emb, const float* lin, const float* bias,
                              float* flat, int64_t ldf, const ctr_planes* x_planes,
                              float* z_lin, int32_t* err_flag, ctr_stream_t stream) {
  CTR_REQUIRE(emb && lin && bias, "ctr_wd_forward: null table pointer");
  CTR_REQUIRE(B >= 0 && F >= 1 && K >= 1 && V >= 1 && V < (int64_t(1) << 31),
              "ctr_wd_forward: bad sizes B=%lld F=%d K=%d V=%lld", (long long)B, F, K,
              (long long)V);
  CTR_REQUIRE(idx_type == CTR_IDX_I32 || idx_type == CTR_IDX_I64, "bad idx_type %d", idx_type);
  if (B == 0) return CTR_OK;  // an empty batch has no id / output storage
  CTR_REQUIRE(idx && z_lin, "ctr_wd_forward: null idx / z_lin");
  CTR_REQUIRE(flat || x_planes, "ctr_wd_forward: neither flat nor planes given");
  const int64_t W = (int64_t)F * K;
  CTR_REQUIRE(!flat || ldf >= W, "ctr_wd_forward: ldf %lld < F*K = %lld", (long long)ldf,
              (long long)W);
  CTR_REQUIRE(!x_planes || (x_planes->data && x_planes->rows >= B && x_planes->cols >= W &&
                            x_planes->ld >= W && (uintptr_t)x_planes->data % 8 == 0 &&
                            x_planes->plane_stride >= x_planes->rows * x_planes->ld),
              "ctr_wd_forward: planes smaller than [B, F*K = %lld]", (long long)W);
  uint16_t* xpl = x_planes ? static_cast<uint16_t*>(x_planes->data) : nullptr;
  const int64_t xld = x_planes ? x_planes->ld : 0;
  const int64_t xps = x_planes ? x_planes->plane_stride : 0;
  // 16-byte pieces where K, the pointers and the strides allow; the alignment selects a
  // path, never a result (every element is copied, every split is the same operations)
  const bool vec = K % 4 == 0 && wd_aligned16(emb) &&
                   (!flat || (wd_aligned16(flat) && ldf % 4 == 0)) &&
                   (!xpl || (xld % 4 == 0 && xps % 4 == 0));
  const int64_t KV = K / (vec ? 4 : 1);
  const int64_t blocks = ceil_div(B * KV, kWdBlock);
  CTR_REQUIRE(blocks <= 0x7fffffffll, "ctr_wd_forward: B*K too large for one launch");
  const unsigned grid = (unsigned)blocks;
  hipStream_t st = as_stream(stream);
  // a block's kWdBlock pieces touch at most (kWdBlock - 1) / KV + 2 examples
  const int64_t per_block = (kWdBlock - 1) / KV + 2;
  const int64_t stage_n = (per_block < B ? per_block : B) * F;
  const size_t stage_bytes = (size_t)stage_n * kWdStageEntry;
  const bool stage = stage_bytes <= kWdStageBytes;
  const size_t lds = stage ? stage_bytes : 0;
  const int sn = stage ? (int)stage_n : 0;
  dispatch_bool(vec, [&](auto v) {
    constexpr int VEC = decltype(v)::value ? 4 : 1;
    dispatch_bool(stage, [&](auto sg) {
      constexpr bool STAGE = decltype(sg)::value;
      if (idx_type == CTR_IDX_I64)
        hipLaunchKernelGGL((wd_forward_kernel<int64_t, VEC, STAGE>), grid, kWdBlock, lds, st,
                           static_cast<const int64_t*>(idx), B, F, K, V, emb, lin, bias, flat,
                           ldf, xpl, xld, xps, z_lin, sn, err_flag);
      else
        hipLaunchKernelGGL((wd_forward_kernel<int32_t, VEC, STAGE>), grid, kWdBlock, lds, st,
                           static_cast<const int32_t*>(idx), B, F, K, V, emb, lin, bias, flat,
                           ldf, xpl, xld, xps, z_lin, sn, err_flag);
    });
  });
  CTR_LAUNCH_CHECK("ctr_wd_forward");
  return CTR_OK;
}
