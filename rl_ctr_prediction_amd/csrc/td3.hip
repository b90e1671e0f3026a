// The hybrid TD3 agent's small kernels (reference src/models/Hybrid_TD3_model_PER.py:111-393):
// BatchNorm1d forward / backward, the exploration and smoothing noise, the action heads, the
// critic loss and the multi-tensor soft update. The Linear layers stay on the GEMMs.
//
// BatchNorm ownership. A block owns kBnTile = 64 consecutive columns and ALL rows. In the
// vector form (VW = 4: N, every row stride and every pointer allow 16-byte accesses) a wave
// reads four rows at a time, 16 lanes x float4 per row; in the scalar form (VW = 1) one row,
// 64 lanes x float. So a lane always accumulates the same VW columns and no sum ever crosses
// lanes. The block's 4 waves x VW row groups split the rows (row r belongs to group r mod G,
// G = 4 VW); each group's per-column partial goes to LDS and 64 threads add the G partials in
// group order. The order depends on nothing but (B, VW): the same bits every run.
// Statistics are two-pass with fp64 accumulators: the mean first, then the sum of squared
// deviations from it, never E[x^2] - E[x]^2. y and dx are evaluated in fp64 from the fp64 mean
// and invstd and rounded once: a column whose mean is large against its spread loses nothing to
// the rounding of the mean, and with two or three rows, where dx's three terms cancel almost
// entirely, nothing to that of invstd (save_mean_lo / save_invstd_lo keep, for the backward,
// the parts of the two that their fp32 values drop). A third pass writes y; the re-reads hit L2
// (a tile is 256 B x B).
// No kernel here uses a float atomic or scratch memory.
#include <math.h>

#include "ctr_common.h"

namespace ctr {

constexpr int kTd3Threads = 256;
constexpr int kTd3Waves = kTd3Threads / kWave;
constexpr int kBnTile = 64;
constexpr int kTd3MaxA = 64;
constexpr int kSoftMaxTensors = 4096;
constexpr int kSoftMaxBlocksX = 64;
constexpr int kNoiseNone = 0, kNoisePtr = 1, kNoiseSeed = 2;

// Unit-normal draw number i of stream `seed` (the formula of include/ctr_hip.h). Every kernel
// that consumes noise calls this one function, so ctr_td3_noise returns the bits they used.
__device__ __forceinline__ float td3_normal(uint64_t seed, uint64_t i) {
#pragma clang fp contract(off)
  const uint32_t h1 = hash_u32(seed, 2 * i), h2 = hash_u32(seed, 2 * i + 1);
  const float u1 = ((float)(h1 >> 8) + 0.5f) * 0x1p-24f;  // (0, 1), exact
  const float u2 = ((float)(h2 >> 8) + 0.5f) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  return r * cosf(6.28318530717958647692f * u2);
}

__device__ __forceinline__ float td3_clamp(float v, float lo, float hi) {
  return fminf(fmaxf(v, lo), hi);
}

template <int VW>
__device__ __forceinline__ void td3_ld(const float* __restrict__ p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}

template <int VW>
__device__ __forceinline__ void td3_st(float* __restrict__ p, const float (&v)[VW]) {
  if constexpr (VW == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// ------------------------------------------------------------------ BatchNorm1d ------
// red[g][c]: group g's partial of tile column c; the result (the G partials added in group
// order) comes back for column `tid` in threads tid < kBnTile, 0 elsewhere.
template <int G>
__device__ __forceinline__ double bn_combine(double (*red)[kBnTile], int tid) {
  __syncthreads();
  double t = 0.0;
  if (tid < kBnTile) {
#pragma unroll
    for (int g = 0; g < G; ++g) t += red[g][tid];
  }
  return t;
}

template <int VW>
__global__ __launch_bounds__(kTd3Threads) void bn_forward_train_kernel(
    int64_t B, int N, const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean,
    float* __restrict__ running_var, float eps, float momentum, int relu, float* __restrict__ y,
    int64_t ldy, float* __restrict__ save_mean, float* __restrict__ save_mean_lo,
    float* __restrict__ save_invstd, float* __restrict__ save_invstd_lo) {
#pragma clang fp contract(off)
  constexpr int LPR = kWave / VW;      // lanes of one row segment
  constexpr int G = kTd3Waves * VW;    // row groups of the block
  __shared__ double red[G][kBnTile];
  __shared__ double s_mean[kBnTile];
  __shared__ double s_inv[kBnTile];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int cl = (lane % LPR) * VW;    // first of this lane's VW tile columns
  const int grp = wave * VW + lane / LPR;
  const int c0 = blockIdx.x * kBnTile + cl;
  const bool on = c0 < N;              // VW == 4: N % 4 == 0, so c0 + 3 < N too
  float v[VW];
  double s[VW];

#pragma unroll
  for (int j = 0; j < VW; ++j) s[j] = 0.0;
  if (on) {
    for (int64_t r = grp; r < B; r += G) {
      td3_ld<VW>(x + r * ldx + c0, v);
#pragma unroll
      for (int j = 0; j < VW; ++j) s[j] += (double)v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) red[grp][cl + j] = s[j];
  double t = bn_combine<G>(red, tid);
  if (tid < kBnTile) s_mean[tid] = t / (double)B;
  __syncthreads();  // s_mean is complete, and every read of red is over

  double m[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    m[j] = s_mean[cl + j];
    s[j] = 0.0;
  }
  if (on) {
    for (int64_t r = grp; r < B; r += G) {
      td3_ld<VW>(x + r * ldx + c0, v);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const double d = (double)v[j] - m[j];
        s[j] += d * d;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) red[grp][cl + j] = s[j];
  t = bn_combine<G>(red, tid);
  if (tid < kBnTile) {
    const int c = blockIdx.x * kBnTile + tid;
    const double var = t / (double)B, mean = s_mean[tid];
    const double inv_d = 1.0 / sqrt(var + (double)eps);
    s_inv[tid] = inv_d;
    if (c < N) {
      const float mean_f = (float)mean, inv = (float)inv_d;
      if (save_mean) save_mean[c] = mean_f;
      if (save_mean_lo) save_mean_lo[c] = (float)(mean - (double)mean_f);
      if (save_invstd) save_invstd[c] = inv;
      if (save_invstd_lo) save_invstd_lo[c] = (float)(inv_d - (double)inv);
      if (running_mean) {
        const float unbiased = (float)(var * ((double)B / (double)(B - 1)));
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean_f;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * unbiased;
      }
    }
  }
  __syncthreads();

  if (!on) return;
  double sc[VW], be[VW];  // y in fp64, rounded once: nothing is lost where the terms cancel
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    sc[j] = s_inv[cl + j] * (double)gamma[c0 + j];
    be[j] = (double)beta[c0 + j];
  }
  for (int64_t r = grp; r < B; r += G) {
    td3_ld<VW>(x + r * ldx + c0, v);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float o = (float)(((double)v[j] - m[j]) * sc[j] + be[j]);
      v[j] = relu ? fmaxf(o, 0.0f) : o;
    }
    td3_st<VW>(y + r * ldy + c0, v);
  }
}

// Eval mode: row-local, the running statistics only read.
template <int VW>
__global__ __launch_bounds__(kTd3Threads) void bn_forward_eval_kernel(
    int64_t B, int N, const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ running_mean,
    const float* __restrict__ running_var, float eps, int relu, float* __restrict__ y,
    int64_t ldy) {
#pragma clang fp contract(off)
  const int cols = N / VW;
  const int64_t total = B * cols, step = (int64_t)gridDim.x * kTd3Threads;
  for (int64_t it = (int64_t)blockIdx.x * kTd3Threads + threadIdx.x; it < total; it += step) {
    const int64_t r = it / cols;
    const int c0 = (int)(it - r * cols) * VW;
    float v[VW];
    td3_ld<VW>(x + r * ldx + c0, v);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float inv = 1.0f / sqrtf(running_var[c0 + j] + eps);
      const float o = (v[j] - running_mean[c0 + j]) * inv * gamma[c0 + j] + beta[c0 + j];
      v[j] = relu ? fmaxf(o, 0.0f) : o;
    }
    td3_st<VW>(y + r * ldy + c0, v);
  }
}

// Training-mode backward. g = dy masked by the ReLU (y > 0, as torch's threshold backward);
// dbeta = sum g, dgamma = sum g * x_hat, dx = gamma * invstd * (g - dbeta / B - x_hat * dgamma / B).
template <int VW>
__global__ __launch_bounds__(kTd3Threads) void bn_backward_kernel(
    int64_t B, int N, const float* __restrict__ dy, int64_t lddy, const float* __restrict__ y,
    int64_t ldy, int relu, const float* __restrict__ x, int64_t ldx,
    const float* __restrict__ save_mean, const float* __restrict__ save_mean_lo,
    const float* __restrict__ save_invstd, const float* __restrict__ save_invstd_lo,
    const float* __restrict__ gamma, float* __restrict__ dgamma, float* __restrict__ dbeta,
    float* __restrict__ dx, int64_t ldd) {
#pragma clang fp contract(off)
  constexpr int LPR = kWave / VW;
  constexpr int G = kTd3Waves * VW;
  __shared__ double red_b[G][kBnTile];
  __shared__ double red_g[G][kBnTile];
  __shared__ double s_kb[kBnTile], s_kg[kBnTile];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int cl = (lane % LPR) * VW;
  const int grp = wave * VW + lane / LPR;
  const int c0 = blockIdx.x * kBnTile + cl;
  const bool on = c0 < N;
  float g[VW], xv[VW], yv[VW];
  double m[VW], inv[VW], sb[VW], sg[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    sb[j] = sg[j] = 0.0;
    m[j] = inv[j] = 0.0;
    yv[j] = 0.0f;
    if (on) {
      m[j] = (double)save_mean[c0 + j] + (save_mean_lo ? (double)save_mean_lo[c0 + j] : 0.0);
      inv[j] = (double)save_invstd[c0 + j] +
               (save_invstd_lo ? (double)save_invstd_lo[c0 + j] : 0.0);
    }
  }
  if (on) {
    for (int64_t r = grp; r < B; r += G) {
      td3_ld<VW>(dy + r * lddy + c0, g);
      td3_ld<VW>(x + r * ldx + c0, xv);
      if (relu) td3_ld<VW>(y + r * ldy + c0, yv);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const double gj = (relu && !(yv[j] > 0.0f)) ? 0.0 : (double)g[j];
        sb[j] += gj;
        sg[j] += gj * (((double)xv[j] - m[j]) * inv[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    red_b[grp][cl + j] = sb[j];
    red_g[grp][cl + j] = sg[j];
  }
  const double tb = bn_combine<G>(red_b, tid);
  const double tg = bn_combine<G>(red_g, tid);
  if (tid < kBnTile) {
    const int c = blockIdx.x * kBnTile + tid;
    s_kb[tid] = tb / (double)B;
    s_kg[tid] = tg / (double)B;
    if (c < N) {
      dbeta[c] = (float)tb;
      dgamma[c] = (float)tg;
    }
  }
  __syncthreads();
  if (!dx || !on) return;  // dx: block-uniform
  // dx in fp64, rounded once: with few rows its three terms cancel almost entirely
  double kb[VW], kg[VW], sc[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    kb[j] = s_kb[cl + j];
    kg[j] = s_kg[cl + j];
    sc[j] = (double)gamma[c0 + j] * inv[j];
  }
  for (int64_t r = grp; r < B; r += G) {
    td3_ld<VW>(dy + r * lddy + c0, g);
    td3_ld<VW>(x + r * ldx + c0, xv);
    if (relu) td3_ld<VW>(y + r * ldy + c0, yv);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const double gj = (relu && !(yv[j] > 0.0f)) ? 0.0 : (double)g[j];
      const double xh = ((double)xv[j] - m[j]) * inv[j];
      g[j] = (float)(sc[j] * (gj - kb[j] - xh * kg[j]));
    }
    td3_st<VW>(dx + r * ldd + c0, g);
  }
}

// ------------------------------------------------------------------------ noise -------
__global__ __launch_bounds__(kTd3Threads) void td3_noise_kernel(int64_t n, uint64_t seed,
                                                                uint64_t offset,
                                                                float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * kTd3Threads;
  for (int64_t i = (int64_t)blockIdx.x * kTd3Threads + threadIdx.x; i < n; i += step)
    out[i] = td3_normal(seed, offset + (uint64_t)i);
}

// element (row, j) of head `head` (0: continuous, 1: discrete) of a [B, A] pair
__device__ __forceinline__ float td3_head_noise(int mode, const float* __restrict__ ptr,
                                                uint64_t seed, int64_t B, int A, int head,
                                                int64_t row, int j) {
  const int64_t e = row * A + j;
  return mode == kNoisePtr ? ptr[e] : td3_normal(seed, (uint64_t)(head * B * A + e));
}

// ------------------------------------------------------------------ action heads ------
// One row per lane. The lane reads back the c_actions it has just stored itself (a thread sees
// its own stores) instead of holding A values in registers.
__global__ __launch_bounds__(kTd3Threads) void td3_act_kernel(
    int64_t B, int A, const float* __restrict__ pre_c, const float* __restrict__ pre_d,
    int64_t ldp, int mode, const float* __restrict__ noise_c, const float* __restrict__ noise_d,
    uint64_t seed, float sigma, float* c_actions, float* __restrict__ c_softmax,
    float* __restrict__ d_actions, int64_t* __restrict__ d_index) {
#pragma clang fp contract(off)
  const int64_t step = (int64_t)gridDim.x * kTd3Threads;
  for (int64_t row = (int64_t)blockIdx.x * kTd3Threads + threadIdx.x; row < B; row += step) {
    float* c_row = c_actions + row * A;
    float mx = -INFINITY;
    for (int j = 0; j < A; ++j) {
      float v = tanhf(pre_c[row * ldp + j]);
      if (mode != kNoiseNone)
        v = td3_clamp(v + td3_head_noise(mode, noise_c, seed, B, A, 0, row, j) * sigma, -1.0f,
                      1.0f);
      c_row[j] = v;
      mx = fmaxf(mx, v);
    }
    if (c_softmax) {
      float sum = 0.0f;
      for (int j = 0; j < A; ++j) sum += expf(c_row[j] - mx);
      for (int j = 0; j < A; ++j) c_softmax[row * A + j] = expf(c_row[j] - mx) / sum;
    }
    float best = -INFINITY;
    int bi = 0;
    for (int j = 0; j < A; ++j) {
      float v = tanhf(pre_d[row * ldp + j]);
      if (mode != kNoiseNone)
        v = td3_clamp(v + td3_head_noise(mode, noise_d, seed, B, A, 1, row, j) * sigma, -1.0f,
                      1.0f);
      d_actions[row * A + j] = v;
      if (v > best) {  // strict: the lowest index among equal values
        best = v;
        bi = j;
      }
    }
    if (d_index) d_index[row] = (int64_t)bi + 1;
  }
}

// ------------------------------------------------------------- target smoothing -------
__global__ __launch_bounds__(kTd3Threads) void td3_smooth_kernel(
    int64_t B, int A, const float* __restrict__ mean_c, const float* __restrict__ mean_d,
    int64_t ldm, int apply_tanh, int mode, const float* __restrict__ noise_c,
    const float* __restrict__ noise_d, uint64_t seed, float* __restrict__ out_c,
    float* __restrict__ out_d, int64_t ldo) {
#pragma clang fp contract(off)
  const int64_t total = B * A, step = (int64_t)gridDim.x * kTd3Threads;
  for (int64_t e = (int64_t)blockIdx.x * kTd3Threads + threadIdx.x; e < total; e += step) {
    const int64_t row = e / A;
    const int j = (int)(e - row * A);
    float c = mean_c[row * ldm + j], d = mean_d[row * ldm + j];
    if (apply_tanh) {
      c = tanhf(c);
      d = tanhf(d);
    }
    const float nc = td3_head_noise(mode, noise_c, seed, B, A, 0, row, j);
    const float nd = td3_head_noise(mode, noise_d, seed, B, A, 1, row, j);
    out_c[row * ldo + j] = td3_clamp(c + td3_clamp(nc * 0.2f, -0.5f, 0.5f), -1.0f, 1.0f);
    out_d[row * ldo + j] = td3_clamp(d + td3_clamp(nd * 0.2f, -0.5f, 0.5f), -1.0f, 1.0f);
  }
}

// ------------------------------------------------------------------ critic loss -------
// One block: thread t adds rows t, t + 256, ... in order, the wave butterfly and then the four
// waves in order: one fixed order for a given B.
__global__ __launch_bounds__(kTd3Threads) void td3_critic_loss_kernel(
    int64_t B, const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ q1_t, const float* __restrict__ q2_t, const float* __restrict__ r,
    int64_t ldr, const float* __restrict__ isw, float gamma, float* __restrict__ q_target,
    float* __restrict__ td, float* __restrict__ loss, float* __restrict__ dq1,
    float* __restrict__ dq2) {
#pragma clang fp contract(off)
  __shared__ double red[kTd3Waves];
  const int tid = threadIdx.x;
  const float inv_b = 1.0f / (float)B;
  double acc = 0.0;
  for (int64_t i = tid; i < B; i += kTd3Threads) {
    const float a = q1[i], b = q2[i], w = isw[i];
    const float qt = r[i * ldr] + gamma * fminf(q1_t[i], q2_t[i]);
    const float e1 = a - qt, e2 = b - qt;
    q_target[i] = qt;
    td[i] = 2.0f * qt - a - b;
    acc += (double)(w * (e1 * e1 + e2 * e2));
    dq1[i] = 2.0f * w * e1 * inv_b;
    dq2[i] = 2.0f * w * e2 * inv_b;
  }
  acc = wave_sum_f64(acc);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) loss[0] = (float)((red[0] + red[1] + red[2] + red[3]) / (double)B);
}

// ------------------------------------------------------------------ soft update -------
// blockIdx.y: the table entry; the blocks of a row stride over its elements. An entry whose
// two pointers are 16-byte aligned moves float4s and a scalar tail, any other scalars.
__global__ __launch_bounds__(kTd3Threads) void soft_update_multi_kernel(
    const ctr_soft_update_entry* __restrict__ table, float one_minus_tau, float tau) {
#pragma clang fp contract(off)
  const ctr_soft_update_entry e = table[blockIdx.y];
  float* __restrict__ t = e.target;
  const float* __restrict__ s = e.source;
  const int64_t n = e.numel;
  const int64_t first = (int64_t)blockIdx.x * kTd3Threads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kTd3Threads;
  int64_t done = 0;
  if ((((uintptr_t)t | (uintptr_t)s) & 15) == 0) {
    const int64_t n4 = n / 4;
    for (int64_t i = first; i < n4; i += step) {
      float4 a = reinterpret_cast<float4*>(t)[i];
      const float4 b = reinterpret_cast<const float4*>(s)[i];
      a.x = a.x * one_minus_tau + b.x * tau;
      a.y = a.y * one_minus_tau + b.y * tau;
      a.z = a.z * one_minus_tau + b.z * tau;
      a.w = a.w * one_minus_tau + b.w * tau;
      reinterpret_cast<float4*>(t)[i] = a;
    }
    done = n4 * 4;
  }
  for (int64_t i = done + first; i < n; i += step) t[i] = t[i] * one_minus_tau + s[i] * tau;
}

}  // namespace ctr

using namespace ctr;

static bool td3_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static unsigned td3_grid(int64_t items) {  // elementwise launches: grid-stride past 4096 blocks
  const int64_t nb = ceil_div(items, kTd3Threads);
  return (unsigned)(nb < 1 ? 1 : nb < 4096 ? nb : 4096);
}

static int td3_check_bn(const char* who, int64_t B, int N) {
  CTR_REQUIRE(B >= 1 && B <= INT32_MAX, "%s: B=%lld outside [1, 2^31)", who, (long long)B);
  CTR_REQUIRE(N >= 1, "%s: N=%d must be positive", who, N);
  return CTR_OK;
}

static int td3_check_heads(const char* who, int64_t B, int A, int mode, const void* nc,
                           const void* nd) {
  CTR_REQUIRE(B >= 1 && B <= INT32_MAX, "%s: B=%lld outside [1, 2^31)", who, (long long)B);
  CTR_REQUIRE(A >= 1 && A <= kTd3MaxA, "%s: A=%d outside [1, %d]", who, A, kTd3MaxA);
  CTR_REQUIRE(mode >= kNoiseNone && mode <= kNoiseSeed,
              "%s: noise_mode %d is none of 0 (none), 1 (pointers), 2 (seed)", who, mode);
  CTR_REQUIRE(mode != kNoisePtr || (nc && nd), "%s: null noise_c / noise_d with noise_mode 1",
              who);
  return CTR_OK;
}

extern "C" int ctr_bn_forward(int64_t B, int N, const float* x, int64_t ldx, const float* gamma,
                              const float* beta, float* running_mean, float* running_var,
                              float eps, float momentum, int training, int relu, float* y,
                              int64_t ldy, float* save_mean, float* save_mean_lo,
                              float* save_invstd, float* save_invstd_lo, ctr_stream_t stream) {
  int rc = td3_check_bn("ctr_bn_forward", B, N);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(x && y && gamma && beta, "ctr_bn_forward: null x / y / gamma / beta");
  CTR_REQUIRE(ldx >= N && ldy >= N, "ctr_bn_forward: row stride (ldx %lld, ldy %lld) < N=%d",
              (long long)ldx, (long long)ldy, N);
  CTR_REQUIRE(eps >= 0.0f, "ctr_bn_forward: eps is negative");
  const bool vec = N % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && td3_al16(x) && td3_al16(y);
  hipStream_t st = as_stream(stream);
  if (training) {
    CTR_REQUIRE(B >= 2, "ctr_bn_forward: training mode needs B >= 2 rows (got %lld): one value "
                "per channel has no variance", (long long)B);
    CTR_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
                "ctr_bn_forward: running_mean and running_var come together or not at all");
    const unsigned grid = (unsigned)ceil_div(N, kBnTile);
    if (vec) {
      hipLaunchKernelGGL(bn_forward_train_kernel<4>, grid, kTd3Threads, 0, st, B, N, x, ldx,
                         gamma, beta, running_mean, running_var, eps, momentum, relu, y, ldy,
                         save_mean, save_mean_lo, save_invstd, save_invstd_lo);
    } else {
      hipLaunchKernelGGL(bn_forward_train_kernel<1>, grid, kTd3Threads, 0, st, B, N, x, ldx,
                         gamma, beta, running_mean, running_var, eps, momentum, relu, y, ldy,
                         save_mean, save_mean_lo, save_invstd, save_invstd_lo);
    }
  } else {
    CTR_REQUIRE(running_mean && running_var,
                "ctr_bn_forward: null running_mean / running_var in eval mode");
    if (vec) {
      hipLaunchKernelGGL(bn_forward_eval_kernel<4>, td3_grid(B * (N / 4)), kTd3Threads, 0, st, B,
                         N, x, ldx, gamma, beta, running_mean, running_var, eps, relu, y, ldy);
    } else {
      hipLaunchKernelGGL(bn_forward_eval_kernel<1>, td3_grid(B * N), kTd3Threads, 0, st, B, N, x,
                         ldx, gamma, beta, running_mean, running_var, eps, relu, y, ldy);
    }
  }
  CTR_LAUNCH_CHECK("ctr_bn_forward");
  return CTR_OK;
}

extern "C" int ctr_bn_backward(int64_t B, int N, const float* dy, int64_t lddy, const float* y,
                               int64_t ldy, int relu, const float* x, int64_t ldx,
                               const float* save_mean, const float* save_mean_lo,
                               const float* save_invstd, const float* save_invstd_lo,
                               const float* gamma, float* dgamma, float* dbeta, float* dx,
                               int64_t ldd, ctr_stream_t stream) {
  int rc = td3_check_bn("ctr_bn_backward", B, N);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(B >= 2, "ctr_bn_backward: the training-mode backward needs B >= 2 rows (got %lld)",
              (long long)B);
  CTR_REQUIRE(dy && x && save_mean && save_invstd && gamma && dgamma && dbeta,
              "ctr_bn_backward: null dy / x / save_mean / save_invstd / gamma / dgamma / dbeta");
  CTR_REQUIRE(!relu || y, "ctr_bn_backward: null y with relu (the mask is y > 0)");
  CTR_REQUIRE(lddy >= N && ldx >= N && (!relu || ldy >= N) && (!dx || ldd >= N),
              "ctr_bn_backward: a row stride (lddy %lld, ldy %lld, ldx %lld, ldd %lld) < N=%d",
              (long long)lddy, (long long)ldy, (long long)ldx, (long long)ldd, N);
  const bool vec = N % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && td3_al16(dy) && td3_al16(x) &&
                   (!relu || (ldy % 4 == 0 && td3_al16(y))) &&
                   (!dx || (ldd % 4 == 0 && td3_al16(dx)));
  const unsigned grid = (unsigned)ceil_div(N, kBnTile);
  hipStream_t st = as_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(bn_backward_kernel<4>, grid, kTd3Threads, 0, st, B, N, dy, lddy, y, ldy,
                       relu, x, ldx, save_mean, save_mean_lo, save_invstd, save_invstd_lo, gamma,
                       dgamma, dbeta, dx, ldd);
  } else {
    hipLaunchKernelGGL(bn_backward_kernel<1>, grid, kTd3Threads, 0, st, B, N, dy, lddy, y, ldy,
                       relu, x, ldx, save_mean, save_mean_lo, save_invstd, save_invstd_lo, gamma,
                       dgamma, dbeta, dx, ldd);
  }
  CTR_LAUNCH_CHECK("ctr_bn_backward");
  return CTR_OK;
}

extern "C" int ctr_td3_noise(int64_t n, uint64_t seed, uint64_t offset, float* out,
                             ctr_stream_t stream) {
  CTR_REQUIRE(n >= 0 && n <= INT32_MAX, "ctr_td3_noise: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(out, "ctr_td3_noise: null out");
  hipLaunchKernelGGL(td3_noise_kernel, td3_grid(n), kTd3Threads, 0, as_stream(stream), n, seed,
                     offset, out);
  CTR_LAUNCH_CHECK("ctr_td3_noise");
  return CTR_OK;
}

extern "C" int ctr_td3_act(int64_t B, int A, const float* pre_c, const float* pre_d, int64_t ldp,
                           int noise_mode, const float* noise_c, const float* noise_d,
                           uint64_t seed, float sigma, float* c_actions, float* c_softmax,
                           float* d_actions, int64_t* d_index, ctr_stream_t stream) {
  int rc = td3_check_heads("ctr_td3_act", B, A, noise_mode, noise_c, noise_d);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(pre_c && pre_d && c_actions && d_actions,
              "ctr_td3_act: null pre_c / pre_d / c_actions / d_actions");
  CTR_REQUIRE(ldp >= A, "ctr_td3_act: row stride ldp %lld < A=%d", (long long)ldp, A);
  hipLaunchKernelGGL(td3_act_kernel, td3_grid(B), kTd3Threads, 0, as_stream(stream), B, A, pre_c,
                     pre_d, ldp, noise_mode, noise_c, noise_d, seed, sigma, c_actions, c_softmax,
                     d_actions, d_index);
  CTR_LAUNCH_CHECK("ctr_td3_act");
  return CTR_OK;
}

extern "C" int ctr_td3_smooth(int64_t B, int A, const float* mean_c, const float* mean_d,
                              int64_t ldm, int apply_tanh, int noise_mode, const float* noise_c,
                              const float* noise_d, uint64_t seed, float* out_c, float* out_d,
                              int64_t ldo, ctr_stream_t stream) {
  int rc = td3_check_heads("ctr_td3_smooth", B, A, noise_mode, noise_c, noise_d);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(noise_mode != kNoiseNone, "ctr_td3_smooth: noise_mode 0 (smoothing adds noise)");
  CTR_REQUIRE(mean_c && mean_d && out_c && out_d,
              "ctr_td3_smooth: null mean_c / mean_d / out_c / out_d");
  CTR_REQUIRE(ldm >= A && ldo >= A, "ctr_td3_smooth: row stride (ldm %lld, ldo %lld) < A=%d",
              (long long)ldm, (long long)ldo, A);
  hipLaunchKernelGGL(td3_smooth_kernel, td3_grid(B * A), kTd3Threads, 0, as_stream(stream), B, A,
                     mean_c, mean_d, ldm, apply_tanh, noise_mode, noise_c, noise_d, seed, out_c,
                     out_d, ldo);
  CTR_LAUNCH_CHECK("ctr_td3_smooth");
  return CTR_OK;
}

extern "C" int ctr_td3_critic_loss(int64_t B, const float* q1, const float* q2,
                                   const float* q1_t, const float* q2_t, const float* r,
                                   int64_t ldr, const float* isw, float gamma, float* q_target,
                                   float* td, float* loss, float* dq1, float* dq2,
                                   ctr_stream_t stream) {
  CTR_REQUIRE(B >= 1 && B <= INT32_MAX, "ctr_td3_critic_loss: B=%lld outside [1, 2^31)",
              (long long)B);
  CTR_REQUIRE(q1 && q2 && q1_t && q2_t && r && isw,
              "ctr_td3_critic_loss: null q1 / q2 / q1_t / q2_t / r / isw");
  CTR_REQUIRE(q_target && td && loss && dq1 && dq2,
              "ctr_td3_critic_loss: null q_target / td / loss / dq1 / dq2");
  CTR_REQUIRE(ldr >= 1, "ctr_td3_critic_loss: reward stride ldr %lld < 1", (long long)ldr);
  hipLaunchKernelGGL(td3_critic_loss_kernel, 1, kTd3Threads, 0, as_stream(stream), B, q1, q2,
                     q1_t, q2_t, r, ldr, isw, gamma, q_target, td, loss, dq1, dq2);
  CTR_LAUNCH_CHECK("ctr_td3_critic_loss");
  return CTR_OK;
}

extern "C" int ctr_soft_update_multi(int count, const ctr_soft_update_entry* table,
                                     int64_t max_numel, double tau, ctr_stream_t stream) {
  CTR_REQUIRE(count >= 1 && count <= kSoftMaxTensors,
              "ctr_soft_update_multi: count=%d outside [1, %d]", count, kSoftMaxTensors);
  CTR_REQUIRE(table, "ctr_soft_update_multi: null table");
  CTR_REQUIRE(max_numel >= 1 && max_numel <= INT32_MAX,
              "ctr_soft_update_multi: max_numel=%lld outside [1, 2^31)", (long long)max_numel);
  CTR_REQUIRE(tau >= 0.0 && tau <= 1.0, "ctr_soft_update_multi: tau=%g outside [0, 1]", tau);
  // the reference's scalars: (1.0 - tau) and tau are doubles that the fp32 multiply rounds
  const float omt = (float)(1.0 - tau), t = (float)tau;
  int64_t bx = ceil_div(max_numel, (int64_t)kTd3Threads * 4);
  bx = bx < 1 ? 1 : bx < kSoftMaxBlocksX ? bx : kSoftMaxBlocksX;
  hipLaunchKernelGGL(soft_update_multi_kernel, dim3((unsigned)bx, (unsigned)count), kTd3Threads, 0,
                     as_stream(stream), table, omt, t);
  CTR_LAUNCH_CHECK("ctr_soft_update_multi");
  return CTR_OK;
}

// ------------------------------------------------------------- struct-form twins ------
#define TD3_OP_NULL(a, who) CTR_REQUIRE(a, who ": null argument struct")

extern "C" int ctr_op_bn_forward(const ctr_bn_forward_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_bn_forward");
  return ctr_bn_forward(a->B, a->N, a->x, a->ldx, a->gamma, a->beta, a->running_mean,
                        a->running_var, a->eps, a->momentum, a->training, a->relu, a->y, a->ldy,
                        a->save_mean, a->save_mean_lo, a->save_invstd, a->save_invstd_lo, stream);
}

extern "C" int ctr_op_bn_backward(const ctr_bn_backward_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_bn_backward");
  return ctr_bn_backward(a->B, a->N, a->dy, a->lddy, a->y, a->ldy, a->relu, a->x, a->ldx,
                         a->save_mean, a->save_mean_lo, a->save_invstd, a->save_invstd_lo, a->gamma,
                         a->dgamma, a->dbeta, a->dx, a->ldd, stream);
}

extern "C" int ctr_op_td3_noise(const ctr_td3_noise_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_td3_noise");
  return ctr_td3_noise(a->n, a->seed, a->offset, a->out, stream);
}

extern "C" int ctr_op_td3_act(const ctr_td3_act_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_td3_act");
  return ctr_td3_act(a->B, a->A, a->pre_c, a->pre_d, a->ldp, a->noise_mode, a->noise_c,
                     a->noise_d, a->seed, a->sigma, a->c_actions, a->c_softmax, a->d_actions,
                     a->d_index, stream);
}

extern "C" int ctr_op_td3_smooth(const ctr_td3_smooth_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_td3_smooth");
  return ctr_td3_smooth(a->B, a->A, a->mean_c, a->mean_d, a->ldm, a->apply_tanh, a->noise_mode,
                        a->noise_c, a->noise_d, a->seed, a->out_c, a->out_d, a->ldo, stream);
}

extern "C" int ctr_op_td3_critic_loss(const ctr_td3_critic_loss_args* a, ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_td3_critic_loss");
  return ctr_td3_critic_loss(a->B, a->q1, a->q2, a->q1_t, a->q2_t, a->r, a->ldr, a->isw,
                             a->gamma, a->q_target, a->td, a->loss, a->dq1, a->dq2, stream);
}

extern "C" int ctr_op_soft_update_multi(const ctr_soft_update_multi_args* a,
                                        ctr_stream_t stream) {
  TD3_OP_NULL(a, "ctr_op_soft_update_multi");
  return ctr_soft_update_multi(a->count, a->table, a->max_numel, a->tau, stream);
}
