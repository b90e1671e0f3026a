// The v10 hybrid TD3 agent's kernels (reference src/models/v10_Hybrid_TD3_model_PER.py): the
// Gumbel-softmax action heads, the rank mask of the continuous actions under the discrete
// choice with its backward through the heads, gradient-norm clipping over a table of tensors,
// the two-column replay memory (memory-wide max, seeded store, update of column 0; its sampler
// is csrc/per.hip's select with the priority transform applied where a priority is read) and
// the eval-mode BatchNorm parameter backward. The Linear layers stay on the GEMMs, the
// training-mode BatchNorm, the critic loss and the soft update on csrc/td3.hip.
//
// Row kernels. A <= 64 columns: a row takes LPR = the next power of two >= A lanes, a wave
// 64 / LPR rows; lane (l % LPR) holds column l % LPR of its row. The row softmax, argmax and
// rank are butterflies / broadcasts over those LPR lanes, run with every lane of the wave
// active (the trip counts are wave-uniform, loads and stores are predicated).
// Reductions that cross blocks (sum of squares, memory max) never hand data from one block to
// another inside a launch: a launch leaves one partial per block, in an order fixed by the
// sizes, and the NEXT launch's blocks each combine the partials in that order (<= 8 KB, from
// L2). The same inputs give the same bits. No float atomic, no scratch memory.
#include <math.h>

#include "ctr_common.h"

namespace ctr {

constexpr int kV10Threads = 256;
constexpr int kV10Waves = kV10Threads / kWave;
constexpr int kV10MaxA = 64;
constexpr int kV10MaxBlocks = 1024;        // partial maxima of the memory max
constexpr int kClipMaxTensors = CTR_GRAD_CLIP_MAX_TENSORS;
constexpr int kClipBlocksX = 16;           // blocks per tensor of the sum of squares
constexpr int kModeAct = 0, kModePlain = 1, kModeRandom = 2, kModeBest = 3;

struct ClipTable {
  ctr_grad_entry e[kClipMaxTensors];
};

__device__ __forceinline__ float v10_clamp(float v, float lo, float hi) {
  return fminf(fmaxf(v, lo), hi);
}

// -log(-log(u + 1e-20) + 1e-20), the reference's Gumbel draw from a uniform u in fp32
__device__ __forceinline__ float v10_gumbel(float u) {
#pragma clang fp contract(off)
  return -logf(-logf(u + 1e-20f) + 1e-20f);
}

template <int LPR>
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// index of the row's largest value, the lowest index among equal values (j: this lane's
// column; lanes past A pass -inf)
template <int LPR>
__device__ __forceinline__ int row_argmax(float v, int j) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) {
    const float ov = __shfl_xor(v, o, kWave);
    const int oj = __shfl_xor(j, o, kWave);
    if (ov > v || (ov == v && oj < j)) {
      v = ov;
      j = oj;
    }
  }
  return j;
}

// softmax of the row's values (lanes past A: on == false)
template <int LPR>
__device__ __forceinline__ float row_softmax(float z, bool on) {
#pragma clang fp contract(off)
  const float mx = row_max<LPR>(on ? z : -INFINITY);
  const float e = on ? expf(z - mx) : 0.0f;
  return e / row_sum<LPR>(e);
}

// -------------------------------------------------------------------- uniforms -------
// u(seed, i): the first uniform of td3_normal's pair at element i, in (0, 1)
__global__ __launch_bounds__(kV10Threads) void v10_uniform_kernel(int64_t n, uint64_t seed,
                                                                  uint64_t offset,
                                                                  float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * kV10Threads;
  for (int64_t i = (int64_t)blockIdx.x * kV10Threads + threadIdx.x; i < n; i += step) {
    const uint32_t h = hash_u32(seed, 2 * (offset + (uint64_t)i));
    out[i] = ((float)(h >> 8) + 0.5f) * 0x1p-24f;
  }
}

// ------------------------------------------------------------------ action heads ------
template <int LPR>
__global__ __launch_bounds__(kV10Threads) void v10_heads_kernel(
    int64_t B, int A, int mode, const float* __restrict__ pre_c, const float* __restrict__ pre_d,
    int64_t ldp, const float* __restrict__ noise_c, const float* __restrict__ noise_d,
    const float* __restrict__ uniform, float temperature, float* __restrict__ c_means,
    float* __restrict__ c_softmax, float* __restrict__ d_action, int64_t* __restrict__ d_index) {
#pragma clang fp contract(off)
  constexpr int RPW = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1), j = lane % LPR;
  const int64_t wave = (int64_t)blockIdx.x * kV10Waves + threadIdx.x / kWave;
  const int64_t step = (int64_t)gridDim.x * kV10Waves * RPW;
  for (int64_t row0 = wave * RPW; row0 < B; row0 += step) {
    const int64_t row = row0 + lane / LPR;
    const bool on = row < B && j < A;
    const int64_t e = row * A + j;
    float cm = 0.0f, lc = 0.0f, zd = 0.0f;
    if (on) {
      if (mode == kModeRandom) {
        cm = v10_clamp(noise_c[e], -1.0f, 1.0f);
        lc = cm;
        zd = noise_d[e];
      } else {
        cm = tanhf(pre_c[row * ldp + j]);
        const float dq = pre_d[row * ldp + j];
        const float g = v10_gumbel(uniform[e]);
        if (mode == kModeAct) {  // x + normal(x, 0.2) as the reference adds it
          lc = cm + (noise_c[e] * 0.2f + cm);
          zd = ((dq + (noise_d[e] * 0.2f + dq)) + g) / temperature;
        } else {
          lc = cm;
          zd = dq + g;
          if (mode == kModePlain) zd = zd / temperature;
        }
      }
      c_means[e] = cm;
    }
    if (c_softmax) {  // wave-uniform
      const float p = row_softmax<LPR>(lc, on);
      if (on) c_softmax[e] = p;
    }
    float val = zd;  // best: the argmax of the logits themselves
    if (mode != kModeBest) {
      val = row_softmax<LPR>(zd, on);
      if (on && d_action) d_action[e] = val;
    }
    const int best = row_argmax<LPR>(on ? val : -INFINITY, j);
    if (on && j == 0 && d_index) d_index[row] = (int64_t)best + 1;
  }
}

// -------------------------------------------------------------------- rank mask -------
// choose = argmax(d) + 1; column m is kept when its rank among the row's c (descending, ties:
// the lower index first) is below choose.
template <int LPR>
__global__ __launch_bounds__(kV10Threads) void v10_rank_mask_kernel(
    int64_t B, int A, const float* __restrict__ d, int64_t ldd, const float* __restrict__ c,
    int64_t ldc, const float* __restrict__ noise, float* __restrict__ out_c,
    float* __restrict__ out_d, int64_t ldo, uint8_t* __restrict__ keep) {
#pragma clang fp contract(off)
  constexpr int RPW = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1), j = lane % LPR, base = lane - j;
  const int64_t wave = (int64_t)blockIdx.x * kV10Waves + threadIdx.x / kWave;
  const int64_t step = (int64_t)gridDim.x * kV10Waves * RPW;
  for (int64_t row0 = wave * RPW; row0 < B; row0 += step) {
    const int64_t row = row0 + lane / LPR;
    const bool on = row < B && j < A;
    const float dv = on ? d[row * ldd + j] : -INFINITY;
    const float cv = on ? c[row * ldc + j] : 0.0f;
    const int choose = row_argmax<LPR>(dv, j) + 1;
    int rank = 0;
    for (int t = 0; t < LPR; ++t) {  // LPR >= A; every lane takes part in the broadcast
      const float ct = __shfl(cv, base + t, kWave);
      if (t < A && (ct > cv || (ct == cv && t < j))) ++rank;
    }
    if (on) {
      const bool k = rank < choose;
      float v = cv;
      if (noise) v = cv + (noise[row * A + j] * 0.2f + cv);
      out_c[row * ldo + j] = k ? v10_clamp(v, -1.0f, 1.0f) : 0.0f;
      if (out_d) out_d[row * ldo + j] = dv;
      if (keep) keep[row * A + j] = k ? 1 : 0;
    }
  }
}

// ------------------------------------------------- actor loss backward through the heads --
// d pre_c = (keep ? g_c : 0  +  reg * 2 c / (B A)) * (1 - c^2)   (c = tanh(pre_c) lies inside
//           the clamp, whose gradient is 1 on [-1, 1])
// d d_q   = p (g_d - sum_j p_j g_d_j) / T  +  reg * 2 d_q / (B A)   (p = softmax((d_q + g) / T))
template <int LPR>
__global__ __launch_bounds__(kV10Threads) void v10_heads_backward_kernel(
    int64_t B, int A, const float* __restrict__ g_c, const float* __restrict__ g_d, int64_t ldg,
    const uint8_t* __restrict__ keep, const float* __restrict__ c_means,
    const float* __restrict__ d_q, int64_t ldq, const float* __restrict__ d_soft,
    float temperature, float reg, float* __restrict__ d_pre_c, float* __restrict__ d_d_q) {
#pragma clang fp contract(off)
  constexpr int RPW = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1), j = lane % LPR;
  const int64_t wave = (int64_t)blockIdx.x * kV10Waves + threadIdx.x / kWave;
  const int64_t step = (int64_t)gridDim.x * kV10Waves * RPW;
  const float rscale = reg * 2.0f / ((float)B * (float)A);
  for (int64_t row0 = wave * RPW; row0 < B; row0 += step) {
    const int64_t row = row0 + lane / LPR;
    const bool on = row < B && j < A;
    const int64_t e = row * A + j;
    const float p = on ? d_soft[e] : 0.0f;
    const float gd = on ? g_d[row * ldg + j] : 0.0f;
    const float dot = row_sum<LPR>(p * gd);
    if (on) {
      const float cm = c_means[e];
      const float gc = keep[e] ? g_c[row * ldg + j] : 0.0f;
      d_pre_c[e] = (gc + rscale * cm) * (1.0f - cm * cm);
      d_d_q[e] = p * (gd - dot) / temperature + rscale * d_q[row * ldq + j];
    }
  }
}

// ------------------------------------------------------------- gradient clipping ------
// block (x, y): tensor y's elements x * 256 + tid, + gridDim.x * 256, ... squared and added in
// fp64 in that order, the wave butterfly, the four waves in order -> partial[y * gridDim.x + x]
__global__ __launch_bounds__(kV10Threads) void grad_sumsq_kernel(ClipTable tab,
                                                                 double* __restrict__ partial) {
  __shared__ double red[kV10Waves];
  const ctr_grad_entry e = tab.e[blockIdx.y];
  const float* __restrict__ g = e.grad;
  const int tid = threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kV10Threads;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kV10Threads + tid; i < e.numel; i += step) {
    const double v = (double)g[i];
    acc += v * v;
  }
  acc = wave_sum_f64(acc);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0)
    partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Every block adds the n_partial partials in one order (thread t: t, t + 256, ...; butterfly;
// waves in order), so every block scales by the same factor: torch's
// clip_grad_norm_, min(1, max_norm / (norm + 1e-6)) in fp32, applied to every element.
__global__ __launch_bounds__(kV10Threads) void grad_clip_scale_kernel(
    ClipTable tab, const double* __restrict__ partial, int n_partial, float max_norm,
    float* __restrict__ norm_out) {
#pragma clang fp contract(off)
  __shared__ double red[kV10Waves];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n_partial; i += kV10Threads) acc += partial[i];
  acc = wave_sum_f64(acc);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
  __syncthreads();
  const float norm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
  if (norm_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) norm_out[0] = norm;
  const float coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
  const ctr_grad_entry e = tab.e[blockIdx.y];
  float* __restrict__ g = e.grad;
  const int64_t step = (int64_t)gridDim.x * kV10Threads;
  for (int64_t i = (int64_t)blockIdx.x * kV10Threads + tid; i < e.numel; i += step)
    g[i] = g[i] * coef;
}

// ------------------------------------------------------------------ v10 memory --------
// block b: the largest of its elements -> partial[b] (fmaxf: a NaN is skipped)
__global__ __launch_bounds__(kV10Threads) void v10_prio_max_kernel(int64_t n,
                                                                   const float* __restrict__ prio,
                                                                   float* __restrict__ partial) {
  __shared__ float red[kV10Waves];
  const int tid = threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kV10Threads;
  float m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * kV10Threads + tid; i < n; i += step)
    m = fmaxf(m, prio[i]);
  m = row_max<kWave>(m);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// memory[(start + i) % N] = transitions[i]; prio2[row] = td2[i] when td2 is given (Memory.add),
// else (seed, reward): seed = 1 when the memory-wide max is 0, else that max
// (store_transition), the reward the row's last column.
__global__ __launch_bounds__(kV10Threads) void v10_store_kernel(
    int64_t N, int T, int64_t start, int64_t n, const float* __restrict__ transitions,
    int64_t ldt, const float* __restrict__ td2, const float* __restrict__ max_partial,
    int n_partial, float* __restrict__ memory, float* __restrict__ prio2,
    float* __restrict__ seed_out) {
  __shared__ float red[kV10Waves];
  const int tid = threadIdx.x;
  float seedv = 0.0f;
  if (!td2) {  // block-uniform
    float m = -INFINITY;
    for (int i = tid; i < n_partial; i += kV10Threads) m = fmaxf(m, max_partial[i]);
    m = row_max<kWave>(m);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    seedv = m == 0.0f ? 1.0f : m;
    if (seed_out && blockIdx.x == 0 && tid == 0) seed_out[0] = seedv;
  }
  const int64_t total = n * T, step = (int64_t)gridDim.x * kV10Threads;
  for (int64_t it = (int64_t)blockIdx.x * kV10Threads + tid; it < total; it += step) {
    const int64_t i = it / T;
    const int c = (int)(it - i * T);
    const int64_t row = (start + i) % N;  // n <= N: every slot is written by one i
    const float v = transitions[i * ldt + c];
    memory[row * T + c] = v;
    if (td2) {
      if (c < 2) prio2[row * 2 + c] = td2[i * 2 + c];
    } else {
      if (c == 0) prio2[row * 2] = seedv;
      if (c == T - 1) prio2[row * 2 + 1] = v;
    }
  }
}

__global__ __launch_bounds__(kV10Threads) void v10_update_kernel(int64_t N, int64_t k,
                                                                 const int64_t* __restrict__ idx,
                                                                 const float* __restrict__ td,
                                                                 float* __restrict__ prio2) {
  const int64_t step = (int64_t)gridDim.x * kV10Threads;
  for (int64_t i = (int64_t)blockIdx.x * kV10Threads + threadIdx.x; i < k; i += step) {
    const int64_t r = idx[i];
    if (r >= 0 && r < N) prio2[2 * r] = td[i];
  }
}

// ------------------------------------------- eval-mode BatchNorm parameter backward ----
// dbeta = sum dy, dgamma = sum dy * x_hat, x_hat = (x - running_mean) / sqrt(running_var +
// eps): a block owns 64 columns and all rows; thread (g, c) adds rows g, g + 4, ... in fp64,
// then the four groups in order.
__global__ __launch_bounds__(kV10Threads) void bn_eval_backward_kernel(
    int64_t B, int N, const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x,
    int64_t ldx, const float* __restrict__ running_mean, const float* __restrict__ running_var,
    float eps, float* __restrict__ dgamma, float* __restrict__ dbeta) {
#pragma clang fp contract(off)
  __shared__ double red_b[kV10Waves][kWave];
  __shared__ double red_g[kV10Waves][kWave];
  const int tid = threadIdx.x, cl = tid & (kWave - 1), grp = tid / kWave;
  const int c = blockIdx.x * kWave + cl;
  double sb = 0.0, sg = 0.0;
  if (c < N) {
    const double m = (double)running_mean[c];
    const double inv = 1.0 / sqrt((double)running_var[c] + (double)eps);
    for (int64_t r = grp; r < B; r += kV10Waves) {
      const double g = (double)dy[r * lddy + c];
      sb += g;
      sg += g * (((double)x[r * ldx + c] - m) * inv);
    }
  }
  red_b[grp][cl] = sb;
  red_g[grp][cl] = sg;
  __syncthreads();
  if (grp == 0 && c < N) {
    dbeta[c] = (float)(((red_b[0][cl] + red_b[1][cl]) + red_b[2][cl]) + red_b[3][cl]);
    dgamma[c] = (float)(((red_g[0][cl] + red_g[1][cl]) + red_g[2][cl]) + red_g[3][cl]);
  }
}

}  // namespace ctr

using namespace ctr;

static unsigned v10_grid(int64_t items) {  // elementwise launches: grid-stride past 4096 blocks
  const int64_t nb = ceil_div(items, kV10Threads);
  return (unsigned)(nb < 1 ? 1 : nb < 4096 ? nb : 4096);
}

static int v10_lpr(int A) {
  int l = 1;
  while (l < A) l <<= 1;
  return l;
}

static unsigned v10_row_grid(int64_t B, int lpr) {
  return v10_grid(ceil_div(B, kWave / lpr) * kWave);
}

static int v10_max_blocks(int64_t n) {  // of the memory max over n floats
  const int64_t nb = ceil_div(n, (int64_t)kV10Threads * 16);
  return (int)(nb < 1 ? 1 : nb < kV10MaxBlocks ? nb : kV10MaxBlocks);
}

static int v10_check_rows(const char* who, int64_t B, int A) {
  CTR_REQUIRE(B >= 1 && B <= INT32_MAX, "%s: B=%lld outside [1, 2^31)", who, (long long)B);
  CTR_REQUIRE(A >= 1 && A <= kV10MaxA, "%s: A=%d outside [1, %d]", who, A, kV10MaxA);
  return CTR_OK;
}

extern "C" int ctr_td3v10_uniform(int64_t n, uint64_t seed, uint64_t offset, float* out,
                                  ctr_stream_t stream) {
  CTR_REQUIRE(n >= 0 && n <= INT32_MAX, "ctr_td3v10_uniform: n=%lld outside [0, 2^31)",
              (long long)n);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(out, "ctr_td3v10_uniform: null out");
  hipLaunchKernelGGL(v10_uniform_kernel, v10_grid(n), kV10Threads, 0, as_stream(stream), n, seed,
                     offset, out);
  CTR_LAUNCH_CHECK("ctr_td3v10_uniform");
  return CTR_OK;
}

extern "C" int ctr_td3v10_heads(int64_t B, int A, int mode, const float* pre_c,
                                const float* pre_d, int64_t ldp, const float* noise_c,
                                const float* noise_d, const float* uniform, float temperature,
                                float* c_means, float* c_softmax, float* d_action,
                                int64_t* d_index, ctr_stream_t stream) {
  int rc = v10_check_rows("ctr_td3v10_heads", B, A);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(mode >= kModeAct && mode <= kModeBest,
              "ctr_td3v10_heads: mode %d is none of 0 (act), 1 (plain), 2 (random), 3 (best)",
              mode);
  CTR_REQUIRE(c_means, "ctr_td3v10_heads: null c_means");
  if (mode == kModeRandom) {
    CTR_REQUIRE(noise_c && noise_d, "ctr_td3v10_heads: null noise_c / noise_d in mode 2");
  } else {
    CTR_REQUIRE(pre_c && pre_d && uniform, "ctr_td3v10_heads: null pre_c / pre_d / uniform");
    CTR_REQUIRE(ldp >= A, "ctr_td3v10_heads: row stride ldp %lld < A=%d", (long long)ldp, A);
    CTR_REQUIRE(mode != kModeAct || (noise_c && noise_d),
                "ctr_td3v10_heads: null noise_c / noise_d in mode 0");
  }
  CTR_REQUIRE(mode == kModeRandom || mode == kModeBest || temperature > 0.0f,
              "ctr_td3v10_heads: temperature %g must be positive", (double)temperature);
  const int lpr = v10_lpr(A);
  hipStream_t st = as_stream(stream);
  dispatch_width(lpr, [&](auto w) {
    hipLaunchKernelGGL(v10_heads_kernel<decltype(w)::value>, v10_row_grid(B, lpr), kV10Threads, 0,
                       st, B, A, mode, pre_c, pre_d, ldp, noise_c, noise_d, uniform, temperature,
                       c_means, c_softmax, d_action, d_index);
  });
  CTR_LAUNCH_CHECK("ctr_td3v10_heads");
  return CTR_OK;
}

extern "C" int ctr_td3v10_rank_mask(int64_t B, int A, const float* d, int64_t ldd, const float* c,
                                    int64_t ldc, const float* noise, float* out_c, float* out_d,
                                    int64_t ldo, uint8_t* keep, ctr_stream_t stream) {
  int rc = v10_check_rows("ctr_td3v10_rank_mask", B, A);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(d && c && out_c, "ctr_td3v10_rank_mask: null d / c / out_c");
  CTR_REQUIRE(ldd >= A && ldc >= A && ldo >= A,
              "ctr_td3v10_rank_mask: a row stride (ldd %lld, ldc %lld, ldo %lld) < A=%d",
              (long long)ldd, (long long)ldc, (long long)ldo, A);
  const int lpr = v10_lpr(A);
  hipStream_t st = as_stream(stream);
  dispatch_width(lpr, [&](auto w) {
    hipLaunchKernelGGL(v10_rank_mask_kernel<decltype(w)::value>, v10_row_grid(B, lpr),
                       kV10Threads, 0, st, B, A, d, ldd, c, ldc, noise, out_c, out_d, ldo, keep);
  });
  CTR_LAUNCH_CHECK("ctr_td3v10_rank_mask");
  return CTR_OK;
}

extern "C" int ctr_td3v10_heads_backward(int64_t B, int A, const float* g_c, const float* g_d,
                                         int64_t ldg, const uint8_t* keep, const float* c_means,
                                         const float* d_q, int64_t ldq, const float* d_soft,
                                         float temperature, float reg, float* d_pre_c,
                                         float* d_d_q, ctr_stream_t stream) {
  int rc = v10_check_rows("ctr_td3v10_heads_backward", B, A);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(g_c && g_d && keep && c_means && d_q && d_soft && d_pre_c && d_d_q,
              "ctr_td3v10_heads_backward: null g_c / g_d / keep / c_means / d_q / d_soft / "
              "d_pre_c / d_d_q");
  CTR_REQUIRE(ldg >= A && ldq >= A,
              "ctr_td3v10_heads_backward: a row stride (ldg %lld, ldq %lld) < A=%d",
              (long long)ldg, (long long)ldq, A);
  CTR_REQUIRE(temperature > 0.0f, "ctr_td3v10_heads_backward: temperature %g must be positive",
              (double)temperature);
  const int lpr = v10_lpr(A);
  hipStream_t st = as_stream(stream);
  dispatch_width(lpr, [&](auto w) {
    hipLaunchKernelGGL(v10_heads_backward_kernel<decltype(w)::value>, v10_row_grid(B, lpr),
                       kV10Threads, 0, st, B, A, g_c, g_d, ldg, keep, c_means, d_q, ldq, d_soft,
                       temperature, reg, d_pre_c, d_d_q);
  });
  CTR_LAUNCH_CHECK("ctr_td3v10_heads_backward");
  return CTR_OK;
}

// ------------------------------------------------------------- gradient clipping ------
static int clip_blocks_x(int64_t max_numel) {
  const int64_t bx = ceil_div(max_numel, (int64_t)kV10Threads * 8);
  return (int)(bx < 1 ? 1 : bx < kClipBlocksX ? bx : kClipBlocksX);
}

static int clip_check(const char* who, int count, const ctr_grad_entry* table, int64_t max_numel,
                      const void* ws, int64_t ws_bytes, ClipTable* tab) {
  CTR_REQUIRE(count >= 1 && count <= kClipMaxTensors, "%s: count=%d outside [1, %d]", who, count,
              kClipMaxTensors);
  CTR_REQUIRE(table, "%s: null table", who);
  CTR_REQUIRE(max_numel >= 1 && max_numel <= INT32_MAX, "%s: max_numel=%lld outside [1, 2^31)",
              who, (long long)max_numel);
  CTR_REQUIRE(ws && ws_bytes >= ctr_grad_clip_workspace_bytes(count),
              "%s: workspace of %lld bytes is null or shorter than "
              "ctr_grad_clip_workspace_bytes(%d) = %lld", who, (long long)ws_bytes, count,
              (long long)ctr_grad_clip_workspace_bytes(count));
  CTR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace is not 8-byte aligned",
              who);
  memset(tab, 0, sizeof(*tab));
  for (int i = 0; i < count; ++i) {
    CTR_REQUIRE(table[i].grad && table[i].numel >= 1 && table[i].numel <= max_numel,
                "%s: table[%d] has a null pointer or numel %lld outside [1, max_numel=%lld]", who,
                i, (long long)table[i].numel, (long long)max_numel);
    tab->e[i] = table[i];
  }
  return CTR_OK;
}

extern "C" int64_t ctr_grad_clip_workspace_bytes(int count) {
  if (count < 1 || count > kClipMaxTensors) return -1;
  return (int64_t)count * kClipBlocksX * (int64_t)sizeof(double);
}

extern "C" int ctr_grad_sumsq(int count, const ctr_grad_entry* table, int64_t max_numel, void* ws,
                              int64_t ws_bytes, ctr_stream_t stream) {
  ClipTable tab;
  int rc = clip_check("ctr_grad_sumsq", count, table, max_numel, ws, ws_bytes, &tab);
  if (rc != CTR_OK) return rc;
  const int bx = clip_blocks_x(max_numel);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)bx, (unsigned)count), kV10Threads, 0,
                     as_stream(stream), tab, static_cast<double*>(ws));
  CTR_LAUNCH_CHECK("ctr_grad_sumsq");
  return CTR_OK;
}

extern "C" int ctr_grad_clip_scale(int count, const ctr_grad_entry* table, int64_t max_numel,
                                   float max_norm, const void* ws, int64_t ws_bytes,
                                   float* norm_out, ctr_stream_t stream) {
  ClipTable tab;
  int rc = clip_check("ctr_grad_clip_scale", count, table, max_numel, ws, ws_bytes, &tab);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(max_norm > 0.0f, "ctr_grad_clip_scale: max_norm %g must be positive",
              (double)max_norm);
  const int bx = clip_blocks_x(max_numel);
  hipLaunchKernelGGL(grad_clip_scale_kernel, dim3((unsigned)bx, (unsigned)count), kV10Threads, 0,
                     as_stream(stream), tab, static_cast<const double*>(ws), bx * count, max_norm,
                     norm_out);
  CTR_LAUNCH_CHECK("ctr_grad_clip_scale");
  return CTR_OK;
}

// ------------------------------------------------------------------ v10 memory --------
extern "C" int ctr_td3v10_store(int64_t N, int T, int64_t start, int64_t n,
                                const float* transitions, int64_t ldt, const float* td2, void* ws,
                                int64_t ws_bytes, float* memory, float* prio2, float* seed_out,
                                ctr_stream_t stream) {
  CTR_REQUIRE(N >= 1 && N <= INT32_MAX, "ctr_td3v10_store: N=%lld outside [1, 2^31)",
              (long long)N);
  CTR_REQUIRE(T >= 2 && T <= 65536, "ctr_td3v10_store: T=%d outside [2, 65536]", T);
  CTR_REQUIRE(start >= 0 && start < N, "ctr_td3v10_store: start=%lld outside [0, N=%lld)",
              (long long)start, (long long)N);
  CTR_REQUIRE(n >= 0 && n <= N, "ctr_td3v10_store: n=%lld outside [0, N=%lld]", (long long)n,
              (long long)N);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(transitions && memory && prio2,
              "ctr_td3v10_store: null transitions / memory / prio2");
  CTR_REQUIRE(ldt >= T, "ctr_td3v10_store: row stride ldt %lld < T=%d", (long long)ldt, T);
  CTR_REQUIRE(td2 || (ws && ws_bytes >= CTR_TD3V10_MAX_WS_BYTES),
              "ctr_td3v10_store: without td2 a workspace of %d bytes is needed for the memory "
              "max (%lld given)", CTR_TD3V10_MAX_WS_BYTES, (long long)ws_bytes);
  CTR_REQUIRE(td2 || (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
              "ctr_td3v10_store: workspace is not 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const int nblk = v10_max_blocks(2 * N);
  float* partial = static_cast<float*>(ws);
  if (!td2) {  // the max of the WHOLE prio2, before any row is written: a launch of its own
    hipLaunchKernelGGL(v10_prio_max_kernel, (unsigned)nblk, kV10Threads, 0, st, 2 * N, prio2,
                       partial);
  }
  hipLaunchKernelGGL(v10_store_kernel, v10_grid(n * T), kV10Threads, 0, st, N, T, start, n,
                     transitions, ldt, td2, partial, nblk, memory, prio2, seed_out);
  CTR_LAUNCH_CHECK("ctr_td3v10_store");
  return CTR_OK;
}

extern "C" int ctr_td3v10_update(int64_t N, int64_t k, const int64_t* idx, const float* td,
                                 float* prio2, ctr_stream_t stream) {
  CTR_REQUIRE(N >= 1 && N <= INT32_MAX, "ctr_td3v10_update: N=%lld outside [1, 2^31)",
              (long long)N);
  CTR_REQUIRE(k >= 0 && k <= INT32_MAX, "ctr_td3v10_update: k=%lld outside [0, 2^31)",
              (long long)k);
  if (k == 0) return CTR_OK;
  CTR_REQUIRE(idx && td && prio2, "ctr_td3v10_update: null idx / td / prio2");
  hipLaunchKernelGGL(v10_update_kernel, v10_grid(k), kV10Threads, 0, as_stream(stream), N, k, idx,
                     td, prio2);
  CTR_LAUNCH_CHECK("ctr_td3v10_update");
  return CTR_OK;
}

extern "C" int ctr_bn_eval_backward(int64_t B, int N, const float* dy, int64_t lddy,
                                    const float* x, int64_t ldx, const float* running_mean,
                                    const float* running_var, float eps, float* dgamma,
                                    float* dbeta, ctr_stream_t stream) {
  CTR_REQUIRE(B >= 1 && B <= INT32_MAX, "ctr_bn_eval_backward: B=%lld outside [1, 2^31)",
              (long long)B);
  CTR_REQUIRE(N >= 1, "ctr_bn_eval_backward: N=%d must be positive", N);
  CTR_REQUIRE(dy && x && running_mean && running_var && dgamma && dbeta,
              "ctr_bn_eval_backward: null dy / x / running_mean / running_var / dgamma / dbeta");
  CTR_REQUIRE(lddy >= N && ldx >= N,
              "ctr_bn_eval_backward: a row stride (lddy %lld, ldx %lld) < N=%d", (long long)lddy,
              (long long)ldx, N);
  CTR_REQUIRE(eps >= 0.0f, "ctr_bn_eval_backward: eps is negative");
  hipLaunchKernelGGL(bn_eval_backward_kernel, (unsigned)ceil_div(N, kWave), kV10Threads, 0,
                     as_stream(stream), B, N, dy, lddy, x, ldx, running_mean, running_var, eps,
                     dgamma, dbeta);
  CTR_LAUNCH_CHECK("ctr_bn_eval_backward");
  return CTR_OK;
}

// ------------------------------------------------------------- struct-form twins ------
#define V10_OP_NULL(a, who) CTR_REQUIRE(a, who ": null argument struct")

extern "C" int ctr_op_td3v10_uniform(const ctr_td3v10_uniform_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_uniform");
  return ctr_td3v10_uniform(a->n, a->seed, a->offset, a->out, stream);
}

extern "C" int ctr_op_td3v10_heads(const ctr_td3v10_heads_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_heads");
  return ctr_td3v10_heads(a->B, a->A, a->mode, a->pre_c, a->pre_d, a->ldp, a->noise_c, a->noise_d,
                          a->uniform, a->temperature, a->c_means, a->c_softmax, a->d_action,
                          a->d_index, stream);
}

extern "C" int ctr_op_td3v10_rank_mask(const ctr_td3v10_rank_mask_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_rank_mask");
  return ctr_td3v10_rank_mask(a->B, a->A, a->d, a->ldd, a->c, a->ldc, a->noise, a->out_c, a->out_d,
                              a->ldo, a->keep, stream);
}

extern "C" int ctr_op_td3v10_heads_backward(const ctr_td3v10_heads_backward_args* a,
                                            ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_heads_backward");
  return ctr_td3v10_heads_backward(a->B, a->A, a->g_c, a->g_d, a->ldg, a->keep, a->c_means,
                                   a->d_q, a->ldq, a->d_soft, a->temperature, a->reg, a->d_pre_c,
                                   a->d_d_q, stream);
}

extern "C" int ctr_op_grad_sumsq(const ctr_grad_sumsq_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_grad_sumsq");
  return ctr_grad_sumsq(a->count, a->table, a->max_numel, a->ws, a->ws_bytes, stream);
}

extern "C" int ctr_op_grad_clip_scale(const ctr_grad_clip_scale_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_grad_clip_scale");
  return ctr_grad_clip_scale(a->count, a->table, a->max_numel, a->max_norm, a->ws, a->ws_bytes,
                             a->norm_out, stream);
}

extern "C" int ctr_op_td3v10_store(const ctr_td3v10_store_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_store");
  return ctr_td3v10_store(a->N, a->T, a->start, a->n, a->transitions, a->ldt, a->td2, a->ws,
                          a->ws_bytes, a->memory, a->prio2, a->seed_out, stream);
}

extern "C" int ctr_op_td3v10_update(const ctr_td3v10_update_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_td3v10_update");
  return ctr_td3v10_update(a->N, a->k, a->idx, a->td, a->prio2, stream);
}

extern "C" int ctr_op_bn_eval_backward(const ctr_bn_eval_backward_args* a, ctr_stream_t stream) {
  V10_OP_NULL(a, "ctr_op_bn_eval_backward");
  return ctr_bn_eval_backward(a->B, a->N, a->dy, a->lddy, a->x, a->ldx, a->running_mean,
                              a->running_var, a->eps, a->dgamma, a->dbeta, stream);
}
