// Outer-product network (OPNN): the MLP input of p_model.OuterPNN (reference
// src/models/p_model.py:202-254) and its backward.
//
// Forward (p_model.py:244-251): with e_f = E[x_bf], s = e_0 + e_1 + ... + e_{F-1} (fp32, field
// order) and kernel the K x K "outer product" transform,
//   cross[b, j] = sum_i (s[b,j] * kernel[i,j]) * s[b,j] = ksum[j] * s[b,j]^2,  ksum = kernel.sum(0)
//   cat[b] = [ flat(e_0..e_{F-1}) (F*K) | cross (K) ]
// — the sum over i never mixes columns, so there is no pair loop: a gather, a field sum, a
// square and a plane write. Backward: given dcat = dL/dcat (the dX GEMM's output),
//   dslot[b*F+f, k] = dcat[b, f*K+k] + ((2*ksum[k]) * s[b,k]) * dcat[b, F*K+k]
// written per slot [B*F, K]; the per-row sums then go through the deterministic segmented
// sum (ctr_segment_sum_rows) exactly like IPNN's. The backward reads dcat, s and ksum only:
// no ids, no table.
//
// Both kernels are bandwidth-bound streams. One thread owns one 16-byte column piece (K % 4
// == 0 and every pointer / stride 16-byte aligned) or one column (any K) of one example and
// walks the F fields: the K columns of an example are independent, so there is no cross-lane
// or cross-wave reduction and no atomic, and the K/4 (or K) threads of an example read and
// write each row as one contiguous run. A thread keeps kFieldsInFlight row loads in flight
// before the first use (see stage_rows_wave in ctr_common.h). The ids: load_row checks each id
// behind a branch, so a thread that walked its F ids itself would wait for F id loads one
// after the other; instead the block's threads resolve the ids of the block's examples (one
// contiguous run of idx) once, in parallel, into LDS, and every thread reads its example's
// rows from there. Blocks whose ids do not fit kStageBytes of LDS (K of a few columns with
// hundreds of fields) walk their ids themselves.
#include "ctr_common.h"

namespace ctr {

constexpr int kFieldsInFlight = 8;
constexpr int kOpnnBlock = 256;
constexpr size_t kStageBytes = 32 * 1024;  // LDS for a block's resolved ids, at most

template <int VEC>
struct opnn_vec;
template <>
struct opnn_vec<1> {
  typedef float type;
};
template <>
struct opnn_vec<4> {
  typedef float4 type;
};

__device__ __forceinline__ float opnn_zero(float) { return 0.f; }
__device__ __forceinline__ float4 opnn_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float opnn_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 opnn_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// ksum * (s * s): two rounded products
__device__ __forceinline__ float opnn_cross(float ks, float s) {
#pragma clang fp contract(off)
  const float q = s * s;
  return ks * q;
}
__device__ __forceinline__ float4 opnn_cross(float4 ks, float4 s) {
  return make_float4(opnn_cross(ks.x, s.x), opnn_cross(ks.y, s.y), opnn_cross(ks.z, s.z),
                     opnn_cross(ks.w, s.w));
}

// (2 * ksum) * s: the factor of dcat's cross column in every slot gradient of the example
__device__ __forceinline__ float opnn_coef(float ks, float s) {
#pragma clang fp contract(off)
  const float t = 2.f * ks;
  return t * s;
}
__device__ __forceinline__ float4 opnn_coef(float4 ks, float4 s) {
  return make_float4(opnn_coef(ks.x, s.x), opnn_coef(ks.y, s.y), opnn_coef(ks.z, s.z),
                     opnn_coef(ks.w, s.w));
}

// d1 + coef * d2: the product rounded before the sum (torch.mul, then the accumulation)
__device__ __forceinline__ float opnn_slot(float d1, float coef, float d2) {
#pragma clang fp contract(off)
  const float t = coef * d2;
  return d1 + t;
}
__device__ __forceinline__ float4 opnn_slot(float4 d1, float4 coef, float4 d2) {
  return make_float4(opnn_slot(d1.x, coef.x, d2.x), opnn_slot(d1.y, coef.y, d2.y),
                     opnn_slot(d1.z, coef.z, d2.z), opnn_slot(d1.w, coef.w, d2.w));
}

// the three bf16 planes of one element / of four consecutive elements at row base xb + col
__device__ __forceinline__ void opnn_store_planes(uint16_t* xb, int64_t ps, float v) {
  uint16_t h3[3];
  psplit1(v, h3);
#pragma unroll
  for (int q = 0; q < 3; ++q) xb[q * ps] = h3[q];
}
__device__ __forceinline__ void opnn_store_planes(uint16_t* xb, int64_t ps, float4 v) {
  store_planes4_at(xb, ps, v);
}

// piece g of the B * KV pieces -> its example; small: B * KV < 2^32 (one 32-bit division)
__device__ __forceinline__ int64_t opnn_example(int64_t g, int KV, bool small) {
  return small ? (int64_t)((uint32_t)g / (uint32_t)KV) : g / KV;
}

// thread -> (example b, first column k of its piece); false past the last piece
template <int VEC>
__device__ __forceinline__ bool opnn_item(int64_t B, int K, int64_t& b, int& k) {
  const int KV = K / VEC;
  const int64_t n = B * KV;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return false;
  b = opnn_example(gid, KV, (n >> 32) == 0);
  k = (int)(gid - b * KV) * VEC;
  return true;
}

template <typename IdxT, int VEC, bool STAGE>
__global__ __launch_bounds__(kOpnnBlock) void opnn_forward_kernel(
    const IdxT* __restrict__ idx, int64_t B, int F, int K, int64_t V,
    const float* __restrict__ emb, const float* __restrict__ ksum, float* __restrict__ cat,
    int64_t ldc, uint16_t* __restrict__ xpl, int64_t xpl_ld, int64_t xpl_ps,
    float* __restrict__ sum_e, int32_t* err) {
  typedef typename opnn_vec<VEC>::type VT;
  extern __shared__ __attribute__((aligned(16))) long long staged_rows[];
  int64_t b0 = 0;
  if (STAGE) {  // the rows of the block's examples b0 .. b1: ids idx[b0*F, (b1+1)*F)
    const int KV = K / VEC;
    const int64_t n = B * KV;
    const bool small = (n >> 32) == 0;
    const int64_t g0 = (int64_t)blockIdx.x * blockDim.x;  // < n: the grid covers n pieces
    const int64_t g1 = (g0 + blockDim.x < n ? g0 + blockDim.x : n) - 1;
    b0 = opnn_example(g0, KV, small);
    const int64_t nid = (opnn_example(g1, KV, small) - b0 + 1) * F;  // host: fits the LDS
    for (int64_t i = threadIdx.x; i < nid; i += blockDim.x)
      staged_rows[i] = (long long)load_row(idx, b0 * F + i, V, err);
    __syncthreads();
  }
  int64_t b;
  int k;
  if (!opnn_item<VEC>(B, K, b, k)) return;  // after the block's only barrier
  const VT ks = *reinterpret_cast<const VT*>(ksum + k);
  float* ob = cat ? cat + b * ldc + k : nullptr;
  uint16_t* xb = xpl ? xpl + b * xpl_ld + k : nullptr;
  const IdxT* ids = idx + b * F;
  const long long* my_rows = staged_rows + (b - b0) * F;
  VT s = opnn_zero(VT());
  for (int f0 = 0; f0 < F; f0 += kFieldsInFlight) {
    int64_t row[kFieldsInFlight];
    VT v[kFieldsInFlight];
#pragma unroll
    for (int u = 0; u < kFieldsInFlight; ++u)
      row[u] = f0 + u >= F ? 0
               : STAGE ? (int64_t)my_rows[f0 + u]
                       : load_row(ids, (int64_t)(f0 + u), V, err);
#pragma unroll
    for (int u = 0; u < kFieldsInFlight; ++u)
      v[u] = f0 + u < F ? *reinterpret_cast<const VT*>(emb + row[u] * K + k) : opnn_zero(VT());
#pragma unroll
    for (int u = 0; u < kFieldsInFlight; ++u) {
      if (f0 + u < F) {  // block-uniform
        const int64_t col = (int64_t)(f0 + u) * K;
        s = opnn_add(s, v[u]);
        if (ob) *reinterpret_cast<VT*>(ob + col) = v[u];
        if (xb) opnn_store_planes(xb + col, xpl_ps, v[u]);
      }
    }
  }
  const VT cross = opnn_cross(ks, s);
  const int64_t col = (int64_t)F * K;
  if (ob) *reinterpret_cast<VT*>(ob + col) = cross;
  if (xb) opnn_store_planes(xb + col, xpl_ps, cross);
  if (sum_e) *reinterpret_cast<VT*>(sum_e + b * K + k) = s;
}

template <int VEC>
__global__ __launch_bounds__(kOpnnBlock) void opnn_backward_kernel(
    int64_t B, int F, int K, const float* __restrict__ sum_e, const float* __restrict__ ksum,
    const float* __restrict__ dcat, int64_t ldd, float* __restrict__ dslot) {
  typedef typename opnn_vec<VEC>::type VT;
  int64_t b;
  int k;
  if (!opnn_item<VEC>(B, K, b, k)) return;
  const float* db = dcat + b * ldd + k;
  const VT ks = *reinterpret_cast<const VT*>(ksum + k);
  const VT s = *reinterpret_cast<const VT*>(sum_e + b * K + k);
  const VT d2 = *reinterpret_cast<const VT*>(db + (int64_t)F * K);
  const VT coef = opnn_coef(ks, s);
  float* out = dslot + b * F * K + k;
  for (int f0 = 0; f0 < F; f0 += kFieldsInFlight) {
    VT d1[kFieldsInFlight];
#pragma unroll
    for (int u = 0; u < kFieldsInFlight; ++u)
      d1[u] = f0 + u < F ? *reinterpret_cast<const VT*>(db + (int64_t)(f0 + u) * K)
                         : opnn_zero(VT());
#pragma unroll
    for (int u = 0; u < kFieldsInFlight; ++u)
      if (f0 + u < F)  // block-uniform
        *reinterpret_cast<VT*>(out + (int64_t)(f0 + u) * K) = opnn_slot(d1[u], coef, d2);
  }
}

}  // namespace ctr

using namespace ctr;

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// grid of kOpnnBlock-thread blocks over B * (K / vec) pieces
static int opnn_grid(int64_t B, int K, int vec, unsigned* grid) {
  const int64_t blocks = ceil_div(B * (K / vec), kOpnnBlock);
  CTR_REQUIRE(blocks <= 0x7fffffffll, "opnn: B*K too large for one launch");
  *grid = (unsigned)blocks;
  return CTR_OK;
}

extern "C" int ctr_opnn_forward(const void* idx, int idx_type, int64_t B, int F, int K,
                                int64_t V, const float* emb, const float* ksum, float* cat,
                                int64_t ldc, const ctr_planes* cat_planes, float* sum_e,
                                int32_t* err_flag, ctr_stream_t stream) {
  CTR_REQUIRE(idx, "ctr_opnn_forward: null idx");
  CTR_REQUIRE(emb, "ctr_opnn_forward: null emb");
  CTR_REQUIRE(ksum, "ctr_opnn_forward: null ksum");
  CTR_REQUIRE(B >= 0 && F >= 1 && K >= 1 && V >= 1,
              "ctr_opnn_forward: bad sizes B=%lld F=%d K=%d V=%lld", (long long)B, F, K,
              (long long)V);
  CTR_REQUIRE(idx_type == CTR_IDX_I32 || idx_type == CTR_IDX_I64, "bad idx_type %d", idx_type);
  CTR_REQUIRE(cat || cat_planes, "ctr_opnn_forward: neither cat nor planes given");
  const int64_t W = (int64_t)F * K + K;
  CTR_REQUIRE(!cat || ldc >= W, "ctr_opnn_forward: ldc %lld < F*K + K = %lld", (long long)ldc,
              (long long)W);
  CTR_REQUIRE(!cat_planes || (cat_planes->data && cat_planes->rows >= B && cat_planes->cols >= W &&
                              cat_planes->ld >= W && (uintptr_t)cat_planes->data % 8 == 0 &&
                              cat_planes->plane_stride >= cat_planes->rows * cat_planes->ld),
              "ctr_opnn_forward: planes smaller than cat [B, %lld]", (long long)W);
  if (B == 0) return CTR_OK;
  uint16_t* xpl = cat_planes ? static_cast<uint16_t*>(cat_planes->data) : nullptr;
  const int64_t xld = cat_planes ? cat_planes->ld : 0;
  const int64_t xps = cat_planes ? cat_planes->plane_stride : 0;
  // 16-byte pieces where K, the pointers and the strides allow; the alignment selects a
  // path, never a result (the same operations per element in the same order)
  const bool vec = K % 4 == 0 && aligned16(emb) && aligned16(ksum) &&
                   (!cat || (aligned16(cat) && ldc % 4 == 0)) &&
                   (!xpl || (xld % 4 == 0 && xps % 4 == 0)) && (!sum_e || aligned16(sum_e));
  unsigned grid;
  int rc = opnn_grid(B, K, vec ? 4 : 1, &grid);
  if (rc != CTR_OK) return rc;
  hipStream_t st = as_stream(stream);
  // a block's kOpnnBlock pieces touch at most (kOpnnBlock - 1) / KV + 2 examples
  const int64_t KV = K / (vec ? 4 : 1);
  const int64_t per_block = (kOpnnBlock - 1) / KV + 2;
  const size_t stage_bytes = (size_t)(per_block < B ? per_block : B) * F * sizeof(long long);
  const bool stage = stage_bytes <= kStageBytes;
  const size_t lds = stage ? stage_bytes : 0;
  dispatch_bool(vec, [&](auto v) {
    constexpr int VEC = decltype(v)::value ? 4 : 1;
    dispatch_bool(stage, [&](auto sg) {
      constexpr bool STAGE = decltype(sg)::value;
      if (idx_type == CTR_IDX_I64)
        hipLaunchKernelGGL((opnn_forward_kernel<int64_t, VEC, STAGE>), grid, kOpnnBlock, lds, st,
                           static_cast<const int64_t*>(idx), B, F, K, V, emb, ksum, cat, ldc,
                           xpl, xld, xps, sum_e, err_flag);
      else
        hipLaunchKernelGGL((opnn_forward_kernel<int32_t, VEC, STAGE>), grid, kOpnnBlock, lds, st,
                           static_cast<const int32_t*>(idx), B, F, K, V, emb, ksum, cat, ldc,
                           xpl, xld, xps, sum_e, err_flag);
    });
  });
  CTR_LAUNCH_CHECK("ctr_opnn_forward");
  return CTR_OK;
}

extern "C" int ctr_opnn_backward(int64_t B, int F, int K, const float* sum_e, const float* ksum,
                                 const float* dcat, int64_t ldd, float* dslot,
                                 ctr_stream_t stream) {
  CTR_REQUIRE(sum_e, "ctr_opnn_backward: null sum_e");
  CTR_REQUIRE(ksum, "ctr_opnn_backward: null ksum");
  CTR_REQUIRE(dcat, "ctr_opnn_backward: null dcat");
  CTR_REQUIRE(dslot, "ctr_opnn_backward: null dslot");
  CTR_REQUIRE(B >= 0 && F >= 1 && K >= 1, "ctr_opnn_backward: bad sizes B=%lld F=%d K=%d",
              (long long)B, F, K);
  const int64_t W = (int64_t)F * K + K;
  CTR_REQUIRE(ldd >= W, "ctr_opnn_backward: ldd %lld < F*K + K = %lld", (long long)ldd,
              (long long)W);
  if (B == 0) return CTR_OK;
  const bool vec = K % 4 == 0 && aligned16(sum_e) && aligned16(ksum) && aligned16(dcat) &&
                   ldd % 4 == 0 && aligned16(dslot);
  unsigned grid;
  int rc = opnn_grid(B, K, vec ? 4 : 1, &grid);
  if (rc != CTR_OK) return rc;
  hipStream_t st = as_stream(stream);
  dispatch_bool(vec, [&](auto v) {
    constexpr int VEC = decltype(v)::value ? 4 : 1;
    hipLaunchKernelGGL((opnn_backward_kernel<VEC>), grid, kOpnnBlock, 0, st, B, F, K, sum_e, ksum, dcat,
                       ldd, dslot);
  });
  CTR_LAUNCH_CHECK("ctr_opnn_backward");
  return CTR_OK;
}
