// Prioritized replay memory of the hybrid TD3 agent (reference
// src/models/Hybrid_TD3_model_PER.py:22-109): add, priority update and the two samplers, with
// storage and selection on the device and no device-to-host copy anywhere.
//
// Sampling. A sequential weighted draw without replacement is, in distribution, the top-k of
// key_i = log p_i + Gumbel_i in descending order (Gumbel top-k); the greedy sampler is the top-k
// of key_i = p_i. Both are one exact selection of the k largest keys of [0, n_valid), ties to
// the lower index, returned in descending key (ties: ascending index) order:
//   1. keys map to uint32 in an order-preserving way (per_ord);
//   2. three streaming passes (digits of 11, 11 and 10 bits, most significant first) count
//      the digit of every element that matches the digits resolved so far in a block-local LDS
//      histogram and flush it with integer atomics; after each pass one block walks the
//      histogram from the top and fixes the next digit. The first pass computes the keys from
//      prio (hash, three logarithms: compute-bound) and keeps their uint32 images in the
//      workspace; the later passes stream those 4 n_valid bytes. After the third pass the
//      threshold key u* is known, with need = the number of elements equal to u* that still
//      belong to the winners;
//   3. every block owns one contiguous index range. A counting pass records each block's keys
//      above u* and equal to u*; the compaction pass stores every element above u* and the
//      first `need` elements equal to u*, each at (counts of the blocks before) + (an ordered
//      scan inside the block). So the ties taken are the lowest indices (fresh transitions all
//      enter with td = 1: whole blocks of equal priorities are the normal case), and no slot
//      comes from an atomic (measured: 4096 returning atomics on one counter take 40 us);
//   4. a rank sort of the k (key, index) pairs, 64-bit words staged in LDS by k / 64 blocks,
//      writes idx; a last launch gathers the rows and computes the importance weights.
// min_p of the filled prefix rides along the first pass (per-block minima, reduced by the
// first pick block).
// Nothing here uses a float atomic and every integer count is exact, so idx, batch and isw are
// the same bits for the same (prio, seed), order included.
#include <math.h>

#include "ctr_common.h"

namespace ctr {

constexpr int kPerMaxK = 8192;
constexpr int kPerThreads = 256;
constexpr int kPerTile = kPerThreads * 4;  // elements of one block iteration (4 per thread)
constexpr int kPerMaxBlocks = 1024;        // blocks of a streaming pass (per-block scratch)
constexpr int kPerBins = 2048;             // 11-bit digits (the last pass: 10 bits, 1024 bins)
constexpr int kPerStochastic = 0, kPerGreedy = 1;

struct PerState {
  uint32_t prefix;    // digits resolved so far; after the third pass the threshold key u*
  int32_t krem;       // winners still to find among the elements that match prefix
  float min_p;
  int32_t pad;
};

// workspace layout (bytes); the part in front of kPerWsZeroed is zeroed by every sample
constexpr int64_t kPerWsHist = 0;                                        // int32 [3][kPerBins]
constexpr int64_t kPerWsState = kPerWsHist + 3 * kPerBins * 4;           // PerState
constexpr int64_t kPerWsZeroed = kPerWsState + 64;
constexpr int64_t kPerWsBlockMin = kPerWsZeroed;                         // float [kPerMaxBlocks]
constexpr int64_t kPerWsCntGt = kPerWsBlockMin + kPerMaxBlocks * 4;      // int32 [kPerMaxBlocks]
constexpr int64_t kPerWsCntEq = kPerWsCntGt + kPerMaxBlocks * 4;         // int32 [kPerMaxBlocks]
constexpr int64_t kPerWsCand = kPerWsCntEq + kPerMaxBlocks * 4;          // uint64 [kPerMaxK]
constexpr int64_t kPerWsKeys = kPerWsCand + (int64_t)kPerMaxK * 8;       // uint32 [N]
static_assert(sizeof(PerState) <= 64 && kPerWsCand % 16 == 0 && kPerWsKeys % 16 == 0,
              "per: workspace layout");

// (|td| + eps) ^ alpha: torch.pow(torch.abs(td) + epsilon, alpha) in fp32
__device__ __forceinline__ float per_priority(float td, float eps, float alpha) {
#pragma clang fp contract(off)
  return powf(fabsf(td) + eps, alpha);
}

// The selection key of element i (the formula of include/ctr_hip.h). ctr_per_keys and the
// select's first pass call this one function, so they see the same bits.
__device__ __forceinline__ float per_key(float p, int mode, uint64_t seed, int64_t i) {
#pragma clang fp contract(off)
  if (!(p > 0.f) || p == INFINITY) return -INFINITY;  // p <= 0, NaN, +inf: picked last
  if (mode == kPerGreedy) return p;
  uint32_t h = hash_u32(seed, (uint64_t)i);
  const int drop = 8 - __clz((int)h);  // keep the 24 leading significant bits: (float)h is exact
  if (drop > 0) h = (h >> drop) << drop;
  const float v = ((float)h + 0.5f) * 0x1p-32f;  // [2^-33, 1 - 2^-24]
  const float e = -log1pf(-v);                   // Exp(1), in [2^-33, 16.7]
  const float key = logf(p) - logf(e);           // log p + Gumbel
  return key == 0.f ? 0.f : key;                 // one zero: the uint order has two
}

// order-preserving float -> uint32 (no NaN reaches it)
__device__ __forceinline__ uint32_t per_ord(float key) {
  const uint32_t b = __float_as_uint(key);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (key, index) -> one word whose descending order is key descending, index ascending
__device__ __forceinline__ uint64_t per_pack(uint32_t u, int64_t i) {
  return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
}

// prio[i0 .. i0+3], 0 past n. VEC: prio 16-byte aligned (i0 is a multiple of 4).
template <bool VEC>
__device__ __forceinline__ void per_ld4(const float* __restrict__ prio, int64_t i0, int64_t n,
                                        float (&p)[4]) {
  if (VEC && i0 + 3 < n) {
    const float4 v = *reinterpret_cast<const float4*>(prio + i0);
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = i0 + j < n ? prio[i0 + j] : 0.f;
}

// The v10 memory's priorities (csrc/td3_v10.hip): prio2 is [N, 2] (signed TD error, reward) and
// the priority of row i is (|prio2[i, 0]| + eps) ^ alpha, evaluated where it is read. Rows
// i0 .. i0+3, 0 past n. VEC: prio2 16-byte aligned (i0 is a multiple of 4: 32 bytes a thread).
template <bool VEC>
__device__ __forceinline__ void per_ld4_v10(const float* __restrict__ prio2, int64_t i0,
                                            int64_t n, float eps, float alpha, float (&p)[4]) {
  float raw[4];
  if (VEC && i0 + 3 < n) {
    const float4 a = *reinterpret_cast<const float4*>(prio2 + 2 * i0);
    const float4 b = *reinterpret_cast<const float4*>(prio2 + 2 * i0 + 4);
    raw[0] = a.x;
    raw[1] = a.z;
    raw[2] = b.x;
    raw[3] = b.z;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[j] = i0 + j < n ? prio2[2 * (i0 + j)] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = i0 + j < n ? per_priority(raw[j], eps, alpha) : 0.f;
}

// one count into the block's LDS histogram; bin < 0: none. Called by whole waves. A wave whose
// lanes all hold one bin (equal priorities) adds once instead of 64 times to one address.
__device__ __forceinline__ void per_hist_add(int32_t* h, int bin) {
  const int first = __builtin_amdgcn_readfirstlane(bin);
  if (__all(bin == first)) {
    if (first >= 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&h[first], kWave);
  } else if (bin >= 0) {
    atomicAdd(&h[bin], 1);
  }
}

// sum over the block (kPerThreads), the same value in every thread (red: 4 ints)
__device__ __forceinline__ int per_block_sum(int v, int32_t* red) {
  v = wave_sum_i32(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  const int r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

// exclusive prefix sum of v over the block's threads in thread order; total: the block's sum
__device__ __forceinline__ int per_block_scan(int v, int32_t* red, int& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += t;
  }
  if (lane == kWave - 1) red[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += red[w];
  total = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return before + inc - v;
}

// ------------------------------------------------------------- add / update / keys ----
template <bool VEC>
__global__ __launch_bounds__(kPerThreads) void per_add_kernel(
    int64_t N, int T, int64_t start, int64_t n, const float* __restrict__ transitions,
    int64_t ldt, const float* __restrict__ td, float eps, float alpha,
    float* __restrict__ memory, float* __restrict__ prio) {
  const int cols = VEC ? T / 4 : T;
  const int64_t total = n * cols, step = (int64_t)gridDim.x * kPerThreads;
  for (int64_t it = (int64_t)blockIdx.x * kPerThreads + threadIdx.x; it < total; it += step) {
    const int64_t i = it / cols;
    const int c = (int)(it - i * cols);
    const int64_t row = (start + i) % N;  // n <= N: every slot is written by one i
    if (VEC) {
      *reinterpret_cast<float4*>(memory + row * T + 4 * c) =
          *reinterpret_cast<const float4*>(transitions + i * ldt + 4 * c);
    } else {
      memory[row * T + c] = transitions[i * ldt + c];
    }
    if (c == 0) {
      const float pn = per_priority(td[i], eps, alpha), old = prio[row];
      prio[row] = (pn > old || pn != pn) ? pn : old;  // torch.max: a NaN stays visible
    }
  }
}

// The driver's per-batch store in one launch: the transition row is packed from its five
// sources straight into its slot ([ids | c_actions | d_values | d_action | reward], the ids and
// the action as floats: round-to-nearest-even, what torch's .float() gives) and the slot takes
// the priority of a fresh transition (td = 1). Plain stores: n <= N, every slot has one writer.
template <typename IdxT, typename ActT>
__global__ __launch_bounds__(kPerThreads) void per_store_step_kernel(
    int64_t N, int T, int64_t start, int64_t n, int F, int A, const IdxT* __restrict__ idx,
    const float* __restrict__ c_actions, int64_t ldc, const float* __restrict__ d_values,
    int64_t ldd, const ActT* __restrict__ d_action, const float* __restrict__ rewards,
    int64_t ldr, float eps, float alpha, float* __restrict__ memory, float* __restrict__ prio) {
  const int64_t total = n * T, step = (int64_t)gridDim.x * kPerThreads;
  for (int64_t it = (int64_t)blockIdx.x * kPerThreads + threadIdx.x; it < total; it += step) {
    const int64_t i = it / T;
    const int c = (int)(it - i * T);
    const int64_t row = (start + i) % N;
    float v;
    if (c < F) v = (float)idx[i * F + c];
    else if (c < F + A) v = c_actions[i * ldc + (c - F)];
    else if (c < F + 2 * A) v = d_values[i * ldd + (c - F - A)];
    else if (c == F + 2 * A) v = (float)d_action[i];
    else v = rewards[i * ldr];  // c == T - 1 (T == F + 2A + 2, checked on the host)
    memory[row * T + c] = v;
    if (c == 0) {
      const float pn = per_priority(1.0f, eps, alpha), old = prio[row];
      prio[row] = (pn > old || pn != pn) ? pn : old;  // as per_add_kernel
    }
  }
}

__global__ __launch_bounds__(kPerThreads) void per_update_kernel(
    int64_t N, int64_t k, const int64_t* __restrict__ idx, const float* __restrict__ td,
    float eps, float alpha, float* __restrict__ prio) {
  const int64_t step = (int64_t)gridDim.x * kPerThreads;
  for (int64_t i = (int64_t)blockIdx.x * kPerThreads + threadIdx.x; i < k; i += step) {
    const int64_t r = idx[i];
    if (r >= 0 && r < N) prio[r] = per_priority(td[i], eps, alpha);
  }
}

// V10: prio is the v10 memory's [N, 2] tensor, transformed where it is read (per_ld4_v10)
template <bool V10>
__global__ __launch_bounds__(kPerThreads) void per_keys_kernel(int64_t n,
                                                               const float* __restrict__ prio,
                                                               int mode, uint64_t seed, float eps,
                                                               float alpha,
                                                               float* __restrict__ keys) {
  const int64_t step = (int64_t)gridDim.x * kPerThreads;
  for (int64_t i = (int64_t)blockIdx.x * kPerThreads + threadIdx.x; i < n; i += step)
    keys[i] = per_key(V10 ? per_priority(prio[2 * i], eps, alpha) : prio[i], mode, seed, i);
}

// --------------------------------------------------------------------- selection ------
// ukeys[i0 .. i0+3] (16-byte aligned: i0 is a multiple of 4), 0 past n
__device__ __forceinline__ void per_ldu4(const uint32_t* __restrict__ ukeys, int64_t i0,
                                         int64_t n, uint32_t (&u)[4]) {
  if (i0 + 3 < n) {
    const uint4 v = *reinterpret_cast<const uint4*>(ukeys + i0);
    u[0] = v.x;
    u[1] = v.y;
    u[2] = v.z;
    u[3] = v.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = i0 + j < n ? ukeys[i0 + j] : 0u;
}

// Pass `pass` (0, 1, 2) of the radix select over the block's index range [b * chunk, ..).
// FIRST (pass 0) computes the keys from prio and keeps their uint32 images in ukeys; the
// later passes and the compaction stream those 4 n_valid bytes instead of recomputing them.
template <bool VEC, bool FIRST, bool V10 = false>
__global__ __launch_bounds__(kPerThreads) void per_hist_kernel(
    int64_t n, int64_t chunk, const float* __restrict__ prio, int mode, uint64_t seed, int pass,
    float eps, float alpha, const PerState* __restrict__ st, uint32_t* __restrict__ ukeys,
    int32_t* __restrict__ hist, float* __restrict__ blockmin) {
  __shared__ int32_t h[kPerBins];
  __shared__ float red[kPerThreads / kWave];
  const int tid = threadIdx.x;
  for (int b = tid; b < kPerBins; b += kPerThreads) h[b] = 0;
  __syncthreads();
  const uint32_t prefix = FIRST ? 0u : st->prefix;
  const int hi_shift = pass == 1 ? 21 : 10;               // pass > 0: the bits below prefix
  const int dshift = pass == 0 ? 21 : pass == 1 ? 10 : 0;  // this pass's digit
  const uint32_t dmask = pass == 2 ? 1023u : 2047u;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  float mn = INFINITY;
  for (int64_t t0 = lo; t0 < hi; t0 += kPerTile) {  // block-uniform trip count
    const int64_t i0 = t0 + 4 * tid;
    uint32_t u[4];
    if (FIRST) {
      float p[4];
      if constexpr (V10) {
        per_ld4_v10<VEC>(prio, i0, hi, eps, alpha, p);
      } else {
        per_ld4<VEC>(prio, i0, hi, p);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u[j] = 0u;
        if (i0 + j < hi) {
          mn = fminf(mn, p[j]);
          u[j] = per_ord(per_key(p[j], mode, seed, i0 + j));
        }
      }
      if (i0 + 3 < hi) {
        *reinterpret_cast<uint4*>(ukeys + i0) = make_uint4(u[0], u[1], u[2], u[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < hi) ukeys[i0 + j] = u[j];
      }
    } else {
      per_ldu4(ukeys, i0, hi, u);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int bin = -1;
      if (i0 + j < hi && (FIRST || (u[j] >> hi_shift) == prefix))
        bin = (int)((u[j] >> dshift) & dmask);
      per_hist_add(h, bin);
    }
  }
  __syncthreads();
  for (int b = tid; b < kPerBins; b += kPerThreads) {
    const int32_t c = h[b];
    if (c) atomicAdd(&hist[b], c);
  }
  if (FIRST) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, kWave));
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = mn;
    __syncthreads();
    if (tid == 0) blockmin[blockIdx.x] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  }
}

// One block: the digit of pass `pass`, from the top of its histogram, and (pass 0) min_p.
__global__ __launch_bounds__(kPerThreads) void per_pick_kernel(int pass, int k, int nblk,
                                                               const int32_t* __restrict__ hist,
                                                               const float* __restrict__ blockmin,
                                                               PerState* __restrict__ st) {
  __shared__ int32_t ts[kPerThreads];
  __shared__ float fm[kPerThreads];
  const int tid = threadIdx.x;
  const int bits = pass == 2 ? 10 : 11;
  const int per = (1 << bits) / kPerThreads;  // consecutive bins of a thread
  int s = 0;
  for (int j = 0; j < per; ++j) s += hist[tid * per + j];
  ts[tid] = s;
  const int krem = pass ? st->krem : k;
  const uint32_t prefix = pass ? st->prefix : 0u;
  __syncthreads();  // every thread has read st before its owner below writes it
  int above = 0;
  for (int t = tid + 1; t < kPerThreads; ++t) above += ts[t];
  if (above < krem && krem <= above + s) {  // exactly one thread: the counts sum to >= krem
    int acc = above;
    for (int j = per - 1; j >= 0; --j) {
      const int c = hist[tid * per + j];
      if (acc + c >= krem) {
        st->prefix = (prefix << bits) | (uint32_t)(tid * per + j);
        st->krem = krem - acc;
        break;
      }
      acc += c;
    }
  }
  if (pass == 0) {
    float mn = INFINITY;
    for (int b = tid; b < nblk; b += kPerThreads) mn = fminf(mn, blockmin[b]);
    fm[tid] = mn;
    __syncthreads();
    for (int o = kPerThreads / 2; o > 0; o >>= 1) {  // fixed-order tree
      if (tid < o) fm[tid] = fminf(fm[tid], fm[tid + o]);
      __syncthreads();
    }
    if (tid == 0) st->min_p = fm[0];
  }
}

// COUNT: the block's numbers of keys above u* and equal to u* -> cnt_gt / cnt_eq [block].
// !COUNT: the winners -> cand[0, k): the keys above u* first, then `need` keys equal to u*,
// each group in index order (slot = the counts of the blocks before + an ordered scan inside
// the block), so the ties taken are the lowest indices and no slot needs an atomic.
template <bool COUNT>
__global__ __launch_bounds__(kPerThreads) void per_compact_kernel(
    int64_t n, int64_t chunk, const uint32_t* __restrict__ ukeys, int k,
    const PerState* __restrict__ st, int32_t* __restrict__ cnt_gt, int32_t* __restrict__ cnt_eq,
    uint64_t* __restrict__ cand) {
  __shared__ int32_t red[kPerThreads / kWave];
  const int tid = threadIdx.x;
  const uint32_t ustar = st->prefix;
  const int need = st->krem;
  const int n_gt = k - need;  // keys above u*
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  int gt_base = 0, eq_base = 0;  // COUNT: this thread's counts; else the ranks before the tile
  if (!COUNT) {
    int g = 0, e = 0;
    for (int b = tid; b < (int)blockIdx.x; b += kPerThreads) {
      g += cnt_gt[b];
      e += cnt_eq[b];
    }
    gt_base = per_block_sum(g, red);
    eq_base = per_block_sum(e, red);
  }
  for (int64_t t0 = lo; t0 < hi; t0 += kPerTile) {  // block-uniform trip count
    const int64_t i0 = t0 + 4 * tid;
    uint32_t u[4];
    per_ldu4(ukeys, i0, hi, u);  // 0 past hi: below u* (no key maps under 0x007fffff)
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gt += u[j] > ustar;
      eq += u[j] == ustar;
    }
    if (COUNT) {
      gt_base += gt;
      eq_base += eq;
      continue;
    }
    if (eq_base >= need && gt_base >= n_gt) break;  // block-uniform: nothing left to place
    int total;  // a tile holds <= 1024 of each: two 16-bit fields
    const int before = per_block_scan(gt | (eq << 16), red, total);
    int gs = gt_base + (before & 0xffff), es = eq_base + (before >> 16);
    gt_base += total & 0xffff;
    eq_base += total >> 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (u[j] > ustar) {
        if (gs < n_gt) cand[gs] = per_pack(u[j], i0 + j);
        ++gs;
      } else if (u[j] == ustar) {
        if (es < need) cand[n_gt + es] = per_pack(u[j], i0 + j);
        ++es;
      }
    }
  }
  if (COUNT) {
    gt_base = per_block_sum(gt_base, red);
    eq_base = per_block_sum(eq_base, red);
    if (tid == 0) {
      cnt_gt[blockIdx.x] = gt_base;
      cnt_eq[blockIdx.x] = eq_base;
    }
  }
}

// Rank sort of the k winners: every block stages all of them in LDS (uint64 [k rounded up to
// even]) and ranks 64 of them, one per lane; its four waves each count a quarter of the
// staged words above the lane's own (#{j : cand[j] > cand[i]} is the element's position: the
// words are distinct, each holds its index). A wave's lanes read the same 16 bytes (a
// broadcast), eight independent reads in flight.
__global__ __launch_bounds__(kPerThreads) void per_rank_kernel(int k,
                                                               const uint64_t* __restrict__ cand,
                                                               int64_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char per_lds_raw[];
  uint64_t* s = reinterpret_cast<uint64_t*>(per_lds_raw);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), q = tid / kWave;
  const int k2 = (k + 1) & ~1;
  for (int i = tid; i < k2; i += kPerThreads) s[i] = i < k ? cand[i] : 0ull;  // 0: below all
  __syncthreads();
  const int i = blockIdx.x * kWave + lane;
  const uint64_t mine = s[i < k ? i : 0];
  const int pairs = k2 / 2, per = (pairs + 3) / 4;
  const int p0 = q * per, p1 = p0 + per < pairs ? p0 + per : pairs;  // wave-uniform
  const ulonglong2* s2 = reinterpret_cast<const ulonglong2*>(s);
  int rank = 0;
#pragma unroll 8
  for (int p = p0; p < p1; ++p) {
    const ulonglong2 v = s2[p];
    rank += (int)(v.x > mine) + (int)(v.y > mine);
  }
  __syncthreads();  // the staged words are dead: their LDS (>= 1 KiB) takes the partial ranks
  int32_t* part = reinterpret_cast<int32_t*>(per_lds_raw);
  part[tid] = rank;
  __syncthreads();
  if (q == 0 && i < k) {
    rank += part[lane + kWave] + part[lane + 2 * kWave] + part[lane + 3 * kWave];
    idx[rank] = (int64_t)(0xFFFFFFFFu - (uint32_t)(mine & 0xFFFFFFFFull));
  }
}

// batch[r, :] = memory[idx[r], :], isw[r] = (prio[idx[r]] / min_p) ^ (-beta)
template <bool VEC, bool V10 = false>
__global__ __launch_bounds__(kPerThreads) void per_gather_kernel(
    int64_t N, int T, int k, const float* __restrict__ memory, const float* __restrict__ prio,
    const int64_t* __restrict__ idx, float beta, float eps, float alpha,
    const PerState* __restrict__ st,
    float* __restrict__ batch, float* __restrict__ isw, float* __restrict__ min_p) {
#pragma clang fp contract(off)
  const int cols = VEC ? T / 4 : T;
  const int64_t total = (int64_t)k * cols, step = (int64_t)gridDim.x * kPerThreads;
  const float mp = st->min_p;
  for (int64_t it = (int64_t)blockIdx.x * kPerThreads + threadIdx.x; it < total; it += step) {
    const int64_t r = it / cols;
    const int c = (int)(it - r * cols);
    int64_t row = idx[r];
    if (row < 0 || row >= N) row = 0;  // cannot happen: the selection's counts are exact
    if (VEC) {
      *reinterpret_cast<float4*>(batch + r * T + 4 * c) =
          *reinterpret_cast<const float4*>(memory + row * T + 4 * c);
    } else {
      batch[r * T + c] = memory[row * T + c];
    }
    if (c == 0)
      isw[r] = powf((V10 ? per_priority(prio[2 * row], eps, alpha) : prio[row]) / mp, -beta);
    if (it == 0 && min_p) min_p[0] = mp;
  }
}

}  // namespace ctr

using namespace ctr;

static bool per_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static unsigned per_grid(int64_t items) {  // elementwise launches: grid-stride past 4096 blocks
  const int64_t nb = ceil_div(items, kPerThreads);
  return (unsigned)(nb < 1 ? 1 : nb < 4096 ? nb : 4096);
}

static int per_check_sizes(const char* who, int64_t N, int T) {
  CTR_REQUIRE(N >= 1 && N <= INT32_MAX, "%s: N=%lld outside [1, 2^31)", who, (long long)N);
  CTR_REQUIRE(T >= 1, "%s: T=%d must be positive", who, T);
  return CTR_OK;
}

static int per_check_mode(const char* who, int mode) {
  CTR_REQUIRE(mode == kPerStochastic || mode == kPerGreedy,
              "%s: mode %d is neither 0 (stochastic) nor 1 (greedy)", who, mode);
  return CTR_OK;
}

extern "C" int64_t ctr_per_workspace_bytes(int64_t N, int k) {
  if (N < 1 || N > INT32_MAX || k < 1 || k > kPerMaxK) return 0;
  return kPerWsKeys + align_up(N * 4, 16);
}

extern "C" int ctr_per_add(int64_t N, int T, int64_t start, int64_t n, const float* transitions,
                           int64_t ldt, const float* td, float eps, float alpha, float* memory,
                           float* prio, ctr_stream_t stream) {
  int rc = per_check_sizes("ctr_per_add", N, T);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(n >= 0 && n <= N, "ctr_per_add: n=%lld outside [0, N=%lld]", (long long)n,
              (long long)N);
  CTR_REQUIRE(start >= 0 && start < N, "ctr_per_add: start=%lld outside [0, N=%lld)",
              (long long)start, (long long)N);
  CTR_REQUIRE(memory && prio, "ctr_per_add: null memory / prio");
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(transitions && td, "ctr_per_add: null transitions / td");
  CTR_REQUIRE(ldt >= T, "ctr_per_add: ldt %lld < T", (long long)ldt);
  const bool vec = T % 4 == 0 && ldt % 4 == 0 && per_al16(transitions) && per_al16(memory);
  hipStream_t st = as_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(per_add_kernel<true>, per_grid(n * (T / 4)), kPerThreads, 0, st, N, T,
                       start, n, transitions, ldt, td, eps, alpha, memory, prio);
  } else {
    hipLaunchKernelGGL(per_add_kernel<false>, per_grid(n * T), kPerThreads, 0, st, N, T, start,
                       n, transitions, ldt, td, eps, alpha, memory, prio);
  }
  CTR_LAUNCH_CHECK("ctr_per_add");
  return CTR_OK;
}

extern "C" int ctr_per_store_step(int64_t N, int T, int64_t start, int64_t n, int F, int A,
                                  const void* idx, int idx_type, const float* c_actions,
                                  int64_t ldc, const float* d_values, int64_t ldd,
                                  const void* d_action, int action_type, const float* rewards,
                                  int64_t ldr, float eps, float alpha, float* memory, float* prio,
                                  ctr_stream_t stream) {
  int rc = per_check_sizes("ctr_per_store_step", N, T);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(F >= 1 && A >= 1 && (int64_t)F + 2 * (int64_t)A + 2 == T,
              "ctr_per_store_step: T=%d is not F + 2A + 2 (F=%d, A=%d)", T, F, A);
  CTR_REQUIRE(n >= 0 && n <= N, "ctr_per_store_step: n=%lld outside [0, N=%lld]", (long long)n,
              (long long)N);
  CTR_REQUIRE(start >= 0 && start < N, "ctr_per_store_step: start=%lld outside [0, N=%lld)",
              (long long)start, (long long)N);
  CTR_REQUIRE(idx_type == CTR_IDX_I32 || idx_type == CTR_IDX_I64, "bad idx_type %d", idx_type);
  CTR_REQUIRE(action_type == CTR_IDX_I32 || action_type == CTR_IDX_I64, "bad action_type %d",
              action_type);
  CTR_REQUIRE(memory && prio, "ctr_per_store_step: null memory / prio");
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(idx && c_actions && d_values && d_action && rewards,
              "ctr_per_store_step: null idx / c_actions / d_values / d_action / rewards");
  CTR_REQUIRE(ldc >= A && ldd >= A && ldr >= 1,
              "ctr_per_store_step: row strides ldc=%lld ldd=%lld (>= A) ldr=%lld (>= 1)",
              (long long)ldc, (long long)ldd, (long long)ldr);
  hipStream_t st = as_stream(stream);
  const unsigned grid = per_grid(n * T);
  const bool i64 = idx_type == CTR_IDX_I64, a64 = action_type == CTR_IDX_I64;
  dispatch_bool(i64, [&](auto wi) {
    dispatch_bool(a64, [&](auto wa) {
      using IdxT = std::conditional_t<decltype(wi)::value, int64_t, int32_t>;
      using ActT = std::conditional_t<decltype(wa)::value, int64_t, int32_t>;
      hipLaunchKernelGGL((per_store_step_kernel<IdxT, ActT>), grid, kPerThreads, 0, st, N, T,
                         start, n, F, A, static_cast<const IdxT*>(idx), c_actions, ldc, d_values,
                         ldd, static_cast<const ActT*>(d_action), rewards, ldr, eps, alpha, memory,
                         prio);
    });
  });
  CTR_LAUNCH_CHECK("ctr_per_store_step");
  return CTR_OK;
}

extern "C" int ctr_per_update(int64_t N, int64_t k, const int64_t* idx, const float* td,
                              float eps, float alpha, float* prio, ctr_stream_t stream) {
  CTR_REQUIRE(N >= 1 && N <= INT32_MAX, "ctr_per_update: N=%lld outside [1, 2^31)",
              (long long)N);
  CTR_REQUIRE(k >= 0, "ctr_per_update: k=%lld is negative", (long long)k);
  CTR_REQUIRE(prio, "ctr_per_update: null prio");
  if (k == 0) return CTR_OK;
  CTR_REQUIRE(idx && td, "ctr_per_update: null idx / td");
  hipLaunchKernelGGL(per_update_kernel, per_grid(k), kPerThreads, 0, as_stream(stream), N, k,
                     idx, td, eps, alpha, prio);
  CTR_LAUNCH_CHECK("ctr_per_update");
  return CTR_OK;
}

extern "C" int ctr_per_keys(int64_t n_valid, const float* prio, int mode, uint64_t seed,
                            float* keys, ctr_stream_t stream) {
  CTR_REQUIRE(n_valid >= 0 && n_valid <= INT32_MAX, "ctr_per_keys: n_valid=%lld outside [0, 2^31)",
              (long long)n_valid);
  int rc = per_check_mode("ctr_per_keys", mode);
  if (rc != CTR_OK) return rc;
  if (n_valid == 0) return CTR_OK;
  CTR_REQUIRE(prio && keys, "ctr_per_keys: null prio / keys");
  hipLaunchKernelGGL(per_keys_kernel<false>, per_grid(n_valid), kPerThreads, 0, as_stream(stream),
                     n_valid, prio, mode, seed, 0.f, 0.f, keys);
  CTR_LAUNCH_CHECK("ctr_per_keys");
  return CTR_OK;
}

extern "C" int ctr_td3v10_keys(int64_t n_valid, const float* prio2, float eps, float alpha,
                               uint64_t seed, float* keys, ctr_stream_t stream) {
  CTR_REQUIRE(n_valid >= 0 && n_valid <= INT32_MAX,
              "ctr_td3v10_keys: n_valid=%lld outside [0, 2^31)", (long long)n_valid);
  if (n_valid == 0) return CTR_OK;
  CTR_REQUIRE(prio2 && keys, "ctr_td3v10_keys: null prio2 / keys");
  hipLaunchKernelGGL(per_keys_kernel<true>, per_grid(n_valid), kPerThreads, 0, as_stream(stream),
                     n_valid, prio2, kPerStochastic, seed, eps, alpha, keys);
  CTR_LAUNCH_CHECK("ctr_td3v10_keys");
  return CTR_OK;
}

// The select, shared by ctr_per_sample (prio [N], V10 false: the code it always ran) and
// ctr_td3v10_sample (prio [N, 2], transformed where it is read by eps and alpha).
template <bool V10>
static int per_sample_impl(const char* who, int64_t N, int T, int64_t n_valid, int k, int mode,
                           uint64_t seed, float beta, float eps, float alpha, const float* memory,
                           const float* prio, int64_t* idx, float* batch, float* isw,
                           float* min_p, void* ws, int64_t ws_bytes, ctr_stream_t stream) {
  int rc = per_check_sizes(who, N, T);
  if (rc != CTR_OK) return rc;
  rc = per_check_mode(who, mode);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(n_valid >= 0 && n_valid <= N, "%s: n_valid=%lld outside [0, N=%lld]", who,
              (long long)n_valid, (long long)N);
  CTR_REQUIRE(k >= 1 && k <= kPerMaxK && k <= n_valid,
              "%s: k=%d outside [1, min(n_valid=%lld, %d)]", who, k, (long long)n_valid,
              kPerMaxK);
  CTR_REQUIRE(memory && prio && idx && batch && isw,
              "%s: null memory / prio / idx / batch / isw", who);
  const int64_t need = ctr_per_workspace_bytes(N, k);
  if (!ws || ws_bytes < need || !per_al16(ws)) {
    set_error("%s: workspace %lld < %lld bytes (or not 16-B aligned)", who,
              (long long)ws_bytes, (long long)need);
    return CTR_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  int32_t* hist = reinterpret_cast<int32_t*>(w + kPerWsHist);
  PerState* state = reinterpret_cast<PerState*>(w + kPerWsState);
  float* blockmin = reinterpret_cast<float*>(w + kPerWsBlockMin);
  int32_t* cnt_gt = reinterpret_cast<int32_t*>(w + kPerWsCntGt);
  int32_t* cnt_eq = reinterpret_cast<int32_t*>(w + kPerWsCntEq);
  uint64_t* cand = reinterpret_cast<uint64_t*>(w + kPerWsCand);
  uint32_t* ukeys = reinterpret_cast<uint32_t*>(w + kPerWsKeys);
  CTR_HIP_CHECK(hipMemsetAsync(w, 0, (size_t)kPerWsZeroed, st));

  // every streaming pass gives block b the index range [b * chunk, (b + 1) * chunk)
  const int64_t tiles = ceil_div(n_valid, kPerTile);
  const int64_t tiles_per_block = ceil_div(tiles, kPerMaxBlocks);
  const int nblk = (int)ceil_div(tiles, tiles_per_block);
  const int64_t chunk = tiles_per_block * kPerTile;
  if (per_al16(prio)) {
    hipLaunchKernelGGL((per_hist_kernel<true, true, V10>), nblk, kPerThreads, 0, st, n_valid,
                       chunk, prio, mode, seed, 0, eps, alpha, state, ukeys, hist, blockmin);
  } else {
    hipLaunchKernelGGL((per_hist_kernel<false, true, V10>), nblk, kPerThreads, 0, st, n_valid,
                       chunk, prio, mode, seed, 0, eps, alpha, state, ukeys, hist, blockmin);
  }
  hipLaunchKernelGGL(per_pick_kernel, 1, kPerThreads, 0, st, 0, k, nblk, hist, blockmin, state);
  for (int pass = 1; pass < 3; ++pass) {
    int32_t* hp = hist + pass * kPerBins;
    hipLaunchKernelGGL((per_hist_kernel<true, false>), nblk, kPerThreads, 0, st, n_valid, chunk,
                       prio, mode, seed, pass, eps, alpha, state, ukeys, hp, blockmin);
    hipLaunchKernelGGL(per_pick_kernel, 1, kPerThreads, 0, st, pass, k, nblk, hp, blockmin,
                       state);
  }
  hipLaunchKernelGGL(per_compact_kernel<true>, nblk, kPerThreads, 0, st, n_valid, chunk, ukeys,
                     k, state, cnt_gt, cnt_eq, cand);
  hipLaunchKernelGGL(per_compact_kernel<false>, nblk, kPerThreads, 0, st, n_valid, chunk, ukeys,
                     k, state, cnt_gt, cnt_eq, cand);
  hipLaunchKernelGGL(per_rank_kernel, (unsigned)ceil_div(k, kWave), kPerThreads,
                     (size_t)(k < 128 ? 128 : (k + 1) & ~1) * sizeof(uint64_t), st, k, cand,
                     idx);
  const bool gvec = T % 4 == 0 && per_al16(memory) && per_al16(batch);
  if (gvec) {
    hipLaunchKernelGGL((per_gather_kernel<true, V10>), per_grid((int64_t)k * (T / 4)),
                       kPerThreads, 0, st, N, T, k, memory, prio, idx, beta, eps, alpha, state,
                       batch, isw, min_p);
  } else {
    hipLaunchKernelGGL((per_gather_kernel<false, V10>), per_grid((int64_t)k * T), kPerThreads, 0,
                       st, N, T, k, memory, prio, idx, beta, eps, alpha, state, batch, isw, min_p);
  }
  CTR_LAUNCH_CHECK(who);
  return CTR_OK;
}

extern "C" int ctr_per_sample(int64_t N, int T, int64_t n_valid, int k, int mode, uint64_t seed,
                              float beta, const float* memory, const float* prio, int64_t* idx,
                              float* batch, float* isw, float* min_p, void* ws, int64_t ws_bytes,
                              ctr_stream_t stream) {
  return per_sample_impl<false>("ctr_per_sample", N, T, n_valid, k, mode, seed, beta, 0.f, 0.f,
                                memory, prio, idx, batch, isw, min_p, ws, ws_bytes, stream);
}

extern "C" int ctr_td3v10_sample(int64_t N, int T, int64_t n_valid, int k, uint64_t seed,
                                 float beta, float eps, float alpha, const float* memory,
                                 const float* prio2, int64_t* idx, float* batch, float* isw,
                                 float* min_p, void* ws, int64_t ws_bytes, ctr_stream_t stream) {
  return per_sample_impl<true>("ctr_td3v10_sample", N, T, n_valid, k, kPerStochastic, seed, beta,
                               eps, alpha, memory, prio2, idx, batch, isw, min_p, ws, ws_bytes,
                               stream);
}

extern "C" int ctr_op_td3v10_keys(const ctr_td3v10_keys_args* a, ctr_stream_t stream) {
  CTR_REQUIRE(a, "ctr_op_td3v10_keys: null argument struct");
  return ctr_td3v10_keys(a->n_valid, a->prio2, a->eps, a->alpha, a->seed, a->keys, stream);
}

extern "C" int ctr_op_td3v10_sample(const ctr_td3v10_sample_args* a, ctr_stream_t stream) {
  CTR_REQUIRE(a, "ctr_op_td3v10_sample: null argument struct");
  return ctr_td3v10_sample(a->N, a->T, a->n_valid, a->k, a->seed, a->beta, a->eps, a->alpha,
                           a->memory, a->prio2, a->idx, a->batch, a->isw, a->min_p, a->ws,
                           a->ws_bytes, stream);
}
