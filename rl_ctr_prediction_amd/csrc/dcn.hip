// Cross network of p_model.DCN (reference src/models/p_model.py:423-435), forward and backward.
//
// Forward, per example (x0 = flat(E[x]) [D], W and b [L, D]):
//   x_0 = x0;  s_i = <x_i, W_i>;  x_{i+1} = (x0 * s_i + b_i) + x_i      (i = 0 .. L-1)
// (that association, mul / add / add rounded apart: the reference's order). Outputs: s [B, L]
// (all the backward needs besides x0), x_L (optional) and z = <x_L, w_tail> (optional: the
// cross half of DCN's final Linear, so neither x_L nor cat[x_L, dn] is materialised).
//
// Backward, given g = dL/dx_L (a matrix gL and / or the rank-1 form gz[b] * w_tail), walks
// i = L-1 .. 0:   t_i = <g, x0>;  dx0 += g * s_i;  g += t_i * W_i;   finally dx0 += g.
// The batch reductions use x_i = x0 * (1 + sum_{j<i} s_j) + sum_{j<i} b_j:
//   dW_i    = sum_b c_i[b] * x0[b] + (sum_b t_i[b]) * sum_{j<i} b_j,  c_i = t_i * (1 + sum_{j<i} s_j)
//   dw_tail = sum_b c_L[b] * x0[b] + (sum_b gz[b])  * sum_{j<L} b_j,  c_L = gz  * (1 + sum_{j<L} s_j)
//   db_i    = sum_b gL[b] + (sum_b gz[b]) * w_tail + sum_{j>i} (sum_b t_j[b]) * W_j
// so the backward needs no x_i at all: every batch sum is a row-weighted column sum of x0 (or
// of gL), taken while the row is on chip.
//
// Kernels. D <= 1792 (specialised on the float4 chunks per lane, NV = 1, 2, 4, 7): one wave per
// example, the row in registers (lane l owns columns 4(l + 64c) .. +3), dots by a lane-strided
// sum and a butterfly. The backward's block (8 waves) also stages its 8 rows in LDS; after a
// barrier every thread adds the 8 rows, in row order, into the column sums of the chunk it
// owns, weighted by the rows' coefficients. Blocks stride over the batch and write one
// partial each; a second launch adds the partials in block order: no float atomics, the
// same bits every run. Any other D: one block per example, columns tiled over the block, the
// per-column state re-derived from x0 (or gL) and the scalars in the same operation order,
// the block's partial sums kept in its workspace slab. A row's s, x_L, z and dx0 depend on
// that row alone (and on D's path), never on B or the row's position.
#include <stdlib.h>

#include "ctr_common.h"

namespace ctr {

constexpr int kDcnMaxL = 8;
constexpr int kDcnMaxNV = 7;         // specialised paths: D <= 256 * kDcnMaxNV
constexpr int kDcnBwdRows = 8;       // waves (= rows per pass) of a backward block
constexpr int kDcnMaxBlocks = 256;   // partial slabs: the workspace does not grow with B
constexpr int kDcnTStride = 16;      // scalar partials per block: sum t_0..t_7, sum gz
constexpr int kDcnCoef = 20;         // per staged row: c_0..c_7, c_L, t_0..t_7, gz

__device__ __forceinline__ float4 dcn_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// columns col .. col+3 of a row of D floats; 0 past D. VEC: D % 4 == 0 and p 16-B aligned.
template <bool VEC>
__device__ __forceinline__ float4 dcn_ld4(const float* __restrict__ p, int col, int D) {
  if (VEC) return col < D ? *reinterpret_cast<const float4*>(p + col) : dcn_zero4();
  float4 v;
  v.x = col < D ? p[col] : 0.f;
  v.y = col + 1 < D ? p[col + 1] : 0.f;
  v.z = col + 2 < D ? p[col + 2] : 0.f;
  v.w = col + 3 < D ? p[col + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void dcn_st4(float* __restrict__ p, int col, int D, float4 v) {
  if (VEC) {
    if (col < D) *reinterpret_cast<float4*>(p + col) = v;
    return;
  }
  if (col < D) p[col] = v.x;
  if (col + 1 < D) p[col + 1] = v.y;
  if (col + 2 < D) p[col + 2] = v.z;
  if (col + 3 < D) p[col + 3] = v.w;
}

__device__ __forceinline__ float dcn_dot4(float acc, float4 a, float4 b) {
  acc += a.x * b.x;
  acc += a.y * b.y;
  acc += a.z * b.z;
  acc += a.w * b.w;
  return acc;
}

// x_{i+1} = (x0 * s + b) + x: torch.mul, add, add
__device__ __forceinline__ float4 dcn_update(float4 x0, float s, float4 b, float4 x) {
#pragma clang fp contract(off)
  float4 r;
  r.x = (x0.x * s + b.x) + x.x;
  r.y = (x0.y * s + b.y) + x.y;
  r.z = (x0.z * s + b.z) + x.z;
  r.w = (x0.w * s + b.w) + x.w;
  return r;
}

__device__ __forceinline__ float4 dcn_axpy4(float a, float4 x, float4 y) {  // a * x + y
  y.x += a * x.x;
  y.y += a * x.y;
  y.z += a * x.z;
  y.w += a * x.w;
  return y;
}

// sum over a 256-thread block, the same value in every thread (red: 4 floats)
__device__ __forceinline__ float dcn_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  const float r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------- forward ----------
template <int NV, bool VEC>
__global__ __launch_bounds__(256) void dcn_forward_kernel(int64_t B, int D, int L,
                                                          const float* __restrict__ x0,
                                                          int64_t ldx,
                                                          const float* __restrict__ W,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ w_tail,
                                                          float* __restrict__ s,
                                                          float* __restrict__ xL, int64_t ldo,
                                                          float* __restrict__ z) {
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += step) {  // wave-uniform
    const float* xr = x0 + b * ldx;
    float4 a[NV], x[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      a[c] = dcn_ld4<VEC>(xr, 4 * (lane + kWave * c), D);
      x[c] = a[c];
    }
    for (int i = 0; i < L; ++i) {
      const float* Wi = W + (int64_t)i * D;
      const float* bi = bias + (int64_t)i * D;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c)
        acc = dcn_dot4(acc, x[c], dcn_ld4<VEC>(Wi, 4 * (lane + kWave * c), D));
      const float si = wave_sum(acc);
      if (lane == 0) s[b * L + i] = si;
#pragma unroll
      for (int c = 0; c < NV; ++c)
        x[c] = dcn_update(a[c], si, dcn_ld4<VEC>(bi, 4 * (lane + kWave * c), D), x[c]);
    }
    if (xL) {
      float* o = xL + b * ldo;
#pragma unroll
      for (int c = 0; c < NV; ++c) dcn_st4<VEC>(o, 4 * (lane + kWave * c), D, x[c]);
    }
    if (z) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NV; ++c)
        acc = dcn_dot4(acc, x[c], dcn_ld4<VEC>(w_tail, 4 * (lane + kWave * c), D));
      acc = wave_sum(acc);
      if (lane == 0) z[b] = acc;
    }
  }
}

// Any D: one block per example; layer i's dot re-derives x_i per column from x0, s_0..s_{i-1}
// and b_0..b_{i-1} (the same updates in the same order), so no per-column state is kept.
template <bool VEC>
__global__ __launch_bounds__(256) void dcn_forward_generic(int64_t B, int D, int L,
                                                           const float* __restrict__ x0,
                                                           int64_t ldx,
                                                           const float* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ w_tail,
                                                           float* __restrict__ s,
                                                           float* __restrict__ xL, int64_t ldo,
                                                           float* __restrict__ z) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xr = x0 + b * ldx;
    float sv[kDcnMaxL];
#pragma unroll
    for (int i = 0; i <= kDcnMaxL; ++i) {  // i == L: the tail (z and / or the x_L store)
      if (i > L) continue;                 // block-uniform
      const bool tail = i == L;
      if (tail && !z && !xL) continue;
      const float* wi = tail ? w_tail : W + (int64_t)i * D;
      float* o = tail && xL ? xL + b * ldo : nullptr;
      float acc = 0.f;
      for (int col = 4 * tid; col < D; col += 4 * 256) {
        const float4 a = dcn_ld4<VEC>(xr, col, D);
        float4 x = a;
#pragma unroll
        for (int j = 0; j < kDcnMaxL; ++j)
          if (j < i && j < L)
            x = dcn_update(a, sv[j], dcn_ld4<VEC>(bias + (int64_t)j * D, col, D), x);
        if (wi) acc = dcn_dot4(acc, x, dcn_ld4<VEC>(wi, col, D));
        if (o) dcn_st4<VEC>(o, col, D, x);
      }
      if (tail && !z) continue;
      const float si = dcn_block_sum(acc, red);
      if (i < kDcnMaxL) sv[i] = si;
      if (tid == 0) {
        if (tail)
          z[b] = si;
        else
          s[b * L + i] = si;
      }
    }
  }
}

// ------------------------------------------------------------------ backward ----------
// Workspace: A [nblk][L+1][D] (c_i-weighted column sums of x0; row L: the w_tail one),
// G [kDcnMaxBlocks][D] (column sums of gL), T [kDcnMaxBlocks][kDcnTStride] (sum t_i, [8] = sum gz).
template <int NV, bool VEC, bool HAS_GL>
__global__ __launch_bounds__(64 * kDcnBwdRows) void dcn_backward_kernel(
    int64_t B, int D, int L, const float* __restrict__ x0, int64_t ldx,
    const float* __restrict__ W, const float* __restrict__ s, const float* __restrict__ gL,
    int64_t ldg, const float* __restrict__ gz, const float* __restrict__ w_tail,
    float* __restrict__ dx0, int64_t ldd, float* __restrict__ pA, float* __restrict__ pG,
    float* __restrict__ pT) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int Dp = NV * 4 * kWave;  // staged row, zero past D
  float* tx = lds;
  float* tg = lds + kDcnBwdRows * Dp;
  float* coef = lds + (HAS_GL ? 2 : 1) * kDcnBwdRows * Dp;
  const int tid = threadIdx.x;
  const int wave = tid / kWave;
  const int lane = tid & (kWave - 1);
  float4 accA[kDcnMaxL], accZ = dcn_zero4(), accG = dcn_zero4();
#pragma unroll
  for (int i = 0; i < kDcnMaxL; ++i) accA[i] = dcn_zero4();
  float tsum = 0.f;
  const int64_t step = (int64_t)gridDim.x * kDcnBwdRows;
  for (int64_t b0 = (int64_t)blockIdx.x * kDcnBwdRows; b0 < B; b0 += step) {
    const int64_t b = b0 + wave;
    if (b < B) {  // wave-uniform: one example per wave
      const float* xr = x0 + b * ldx;
      float4 a[NV], g[NV], dx[NV];
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const int col = 4 * (lane + kWave * c);
        a[c] = dcn_ld4<VEC>(xr, col, D);
        *reinterpret_cast<float4*>(tx + wave * Dp + col) = a[c];
        g[c] = dcn_zero4();
        if (HAS_GL) {
          g[c] = dcn_ld4<VEC>(gL + b * ldg, col, D);
          *reinterpret_cast<float4*>(tg + wave * Dp + col) = g[c];
        }
        dx[c] = dcn_zero4();
      }
      const float gzb = gz ? gz[b] : 0.f;
      if (gz) {
#pragma unroll
        for (int c = 0; c < NV; ++c)
          g[c] = dcn_axpy4(gzb, dcn_ld4<VEC>(w_tail, 4 * (lane + kWave * c), D), g[c]);
      }
      const float* sb = s + b * L;
      float* cf = coef + wave * kDcnCoef;
      for (int i = kDcnMaxL - 1; i >= L; --i)
        if (lane == 0) {
          cf[i] = 0.f;
          cf[9 + i] = 0.f;
        }
      for (int i = L - 1; i >= 0; --i) {  // a runtime walk: unrolled, the W loads hoist and spill
        const float* Wi = W + (int64_t)i * D;
        const float si = sb[i];
        float pre = 1.f;  // 1 + s_0 + .. + s_{i-1}
        for (int j = 0; j < i; ++j) pre += sb[j];
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) acc = dcn_dot4(acc, g[c], a[c]);
        const float t = wave_sum(acc);
#pragma unroll
        for (int c = 0; c < NV; ++c) {
          dx[c] = dcn_axpy4(si, g[c], dx[c]);
          g[c] = dcn_axpy4(t, dcn_ld4<VEC>(Wi, 4 * (lane + kWave * c), D), g[c]);
        }
        if (lane == 0) {
          cf[i] = t * pre;
          cf[9 + i] = t;
        }
      }
      float run = 1.f;
      for (int j = 0; j < L; ++j) run += sb[j];
      if (lane == 0) {
        cf[8] = gzb * run;
        cf[17] = gzb;
      }
      float* o = dx0 + b * ldd;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        float4 r = dx[c];
        r.x += g[c].x;
        r.y += g[c].y;
        r.z += g[c].z;
        r.w += g[c].w;
        dcn_st4<VEC>(o, 4 * (lane + kWave * c), D, r);
      }
    }
    __syncthreads();
    const int nrows = B - b0 < kDcnBwdRows ? (int)(B - b0) : kDcnBwdRows;
    if (tid < NV * kWave) {  // the column chunk this thread owns; rows in order
      for (int r = 0; r < nrows; ++r) {
        const float4 xv = *reinterpret_cast<const float4*>(tx + r * Dp + 4 * tid);
        const float* cr = coef + r * kDcnCoef;
#pragma unroll
        for (int i = 0; i < kDcnMaxL; ++i)
          if (i < L) accA[i] = dcn_axpy4(cr[i], xv, accA[i]);
        accZ = dcn_axpy4(cr[8], xv, accZ);
        if (HAS_GL) {
          const float4 gv = *reinterpret_cast<const float4*>(tg + r * Dp + 4 * tid);
          accG.x += gv.x;
          accG.y += gv.y;
          accG.z += gv.z;
          accG.w += gv.w;
        }
      }
    }
    if (tid < 9)
      for (int r = 0; r < nrows; ++r) tsum += coef[r * kDcnCoef + 9 + tid];
    __syncthreads();
  }
  float* A = pA + (int64_t)blockIdx.x * (L + 1) * D;
#pragma unroll
  for (int i = 0; i < kDcnMaxL; ++i)
    if (i < L) dcn_st4<VEC>(A + (int64_t)i * D, 4 * tid, D, accA[i]);
  dcn_st4<VEC>(A + (int64_t)L * D, 4 * tid, D, accZ);
  if (HAS_GL) dcn_st4<VEC>(pG + (int64_t)blockIdx.x * D, 4 * tid, D, accG);
  if (tid < 9) pT[blockIdx.x * kDcnTStride + tid] = tsum;
}

// Any D: one block per example. g at layer i is re-derived per column from g_L and
// t_{L-1}..t_{i+1} (the same updates in the same order); the block's column sums live in its
// workspace slab (each thread owns its columns: plain read-modify-write, rows in order).
template <bool VEC>
__global__ __launch_bounds__(256) void dcn_backward_generic(
    int64_t B, int D, int L, const float* __restrict__ x0, int64_t ldx,
    const float* __restrict__ W, const float* __restrict__ s, const float* __restrict__ gL,
    int64_t ldg, const float* __restrict__ gz, const float* __restrict__ w_tail,
    float* __restrict__ dx0, int64_t ldd, float* __restrict__ pA, float* __restrict__ pG,
    float* __restrict__ pT) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float* A = pA + (int64_t)blockIdx.x * (L + 1) * D;
  float* G = pG + (int64_t)blockIdx.x * D;
  for (int col = 4 * tid; col < D; col += 4 * 256) {
    for (int i = 0; i <= L; ++i) dcn_st4<VEC>(A + (int64_t)i * D, col, D, dcn_zero4());
    if (gL) dcn_st4<VEC>(G, col, D, dcn_zero4());
  }
  float tacc[kDcnMaxL + 1];
#pragma unroll
  for (int i = 0; i <= kDcnMaxL; ++i) tacc[i] = 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xr = x0 + b * ldx;
    const float* gr = gL ? gL + b * ldg : nullptr;
    const float gzb = gz ? gz[b] : 0.f;
    float sv[kDcnMaxL], pre[kDcnMaxL], tv[kDcnMaxL];
    float run = 1.f;
#pragma unroll
    for (int i = 0; i < kDcnMaxL; ++i) {
      sv[i] = i < L ? s[b * L + i] : 0.f;
      pre[i] = run;
      run += sv[i];
      tv[i] = 0.f;
    }
#pragma unroll
    for (int ii = 0; ii < kDcnMaxL; ++ii) {  // t_i = <g at layer i, x0>, i = L-1 .. 0
      const int i = kDcnMaxL - 1 - ii;
      if (i >= L) continue;  // block-uniform
      float acc = 0.f;
      for (int col = 4 * tid; col < D; col += 4 * 256) {
        float4 g = gr ? dcn_ld4<VEC>(gr, col, D) : dcn_zero4();
        if (gz) g = dcn_axpy4(gzb, dcn_ld4<VEC>(w_tail, col, D), g);
#pragma unroll
        for (int jj = 0; jj < kDcnMaxL; ++jj) {
          const int j = kDcnMaxL - 1 - jj;
          if (j > i && j < L) g = dcn_axpy4(tv[j], dcn_ld4<VEC>(W + (int64_t)j * D, col, D), g);
        }
        acc = dcn_dot4(acc, g, dcn_ld4<VEC>(xr, col, D));
      }
      tv[i] = dcn_block_sum(acc, red);
      tacc[i] += tv[i];
    }
    tacc[kDcnMaxL] += gzb;
    float* o = dx0 + b * ldd;
    for (int col = 4 * tid; col < D; col += 4 * 256) {
      const float4 a = dcn_ld4<VEC>(xr, col, D);
      float4 g = dcn_zero4();
      if (gr) {
        g = dcn_ld4<VEC>(gr, col, D);
        float4 q = dcn_ld4<VEC>(G, col, D);
        q.x += g.x;
        q.y += g.y;
        q.z += g.z;
        q.w += g.w;
        dcn_st4<VEC>(G, col, D, q);
      }
      if (gz) g = dcn_axpy4(gzb, dcn_ld4<VEC>(w_tail, col, D), g);
      float4 dx = dcn_zero4();
#pragma unroll
      for (int ii = 0; ii < kDcnMaxL; ++ii) {
        const int i = kDcnMaxL - 1 - ii;
        if (i < L) {
          dx = dcn_axpy4(sv[i], g, dx);
          g = dcn_axpy4(tv[i], dcn_ld4<VEC>(W + (int64_t)i * D, col, D), g);
          float* Ai = A + (int64_t)i * D;
          dcn_st4<VEC>(Ai, col, D, dcn_axpy4(tv[i] * pre[i], a, dcn_ld4<VEC>(Ai, col, D)));
        }
      }
      dx.x += g.x;
      dx.y += g.y;
      dx.z += g.z;
      dx.w += g.w;
      dcn_st4<VEC>(o, col, D, dx);
      float* AL = A + (int64_t)L * D;
      dcn_st4<VEC>(AL, col, D, dcn_axpy4(gzb * run, a, dcn_ld4<VEC>(AL, col, D)));
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i <= kDcnMaxL; ++i) pT[blockIdx.x * kDcnTStride + i] = tacc[i];
  }
}

// Partials -> dW, dw_tail, dbias. Block = 64 columns x 16 groups of consecutive slabs; the
// groups' sums are added in group order. blockIdx.y: 0..L-1 dW_i, L dw_tail, L+1 dbias.
__global__ __launch_bounds__(1024) void dcn_backward_finalize(
    int D, int L, int nblk, const float* __restrict__ pA, const float* __restrict__ pG,
    const float* __restrict__ pT, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ w_tail, float* __restrict__ dW, float* __restrict__ dbias,
    float* __restrict__ dw_tail) {
  __shared__ float red[16][kWave];
  __shared__ float T[9];
  const int tid = threadIdx.x;
  const int cx = tid & (kWave - 1), gy = tid / kWave;
  const int col = blockIdx.x * kWave + cx;
  const int y = blockIdx.y;
  if (tid < 9) {
    float a = 0.f;
    for (int k = 0; k < nblk; ++k) a += pT[k * kDcnTStride + tid];
    T[tid] = a;
  }
  const int per = (nblk + 15) / 16;
  const int k0 = gy * per, k1 = k0 + per < nblk ? k0 + per : nblk;
  float acc = 0.f;
  if (col < D) {
    const float* src = y <= L ? pA + (int64_t)y * D + col : (pG ? pG + col : nullptr);
    const int64_t ld = y <= L ? (int64_t)(L + 1) * D : D;
    if (src)
      for (int k = k0; k < k1; ++k) acc += src[k * ld];
  }
  red[gy][cx] = acc;
  __syncthreads();
  if (gy != 0 || col >= D) return;
  float v = 0.f;
#pragma unroll
  for (int g = 0; g < 16; ++g) v += red[g][cx];
  if (y <= L) {
    float bs = 0.f;
    for (int j = 0; j < y; ++j) bs += bias[(int64_t)j * D + col];
    if (y < L)
      dW[(int64_t)y * D + col] = v + T[y] * bs;
    else if (dw_tail)
      dw_tail[col] = v + T[8] * bs;
  } else {
    if (w_tail) v += T[8] * w_tail[col];
    for (int i = L - 1; i >= 0; --i) {
      dbias[(int64_t)i * D + col] = v;
      v += T[i] * W[(int64_t)i * D + col];
    }
  }
}

}  // namespace ctr

using namespace ctr;

static bool dcn_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int dcn_nv(int D) {  // chunks per lane of the specialised kernels; 0: the generic path
  const int need = (int)ceil_div(D, 4 * kWave);
  if (getenv("CTR_DCN_GENERIC")) return 0;  // A/B runs and tests
  return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= kDcnMaxNV ? kDcnMaxNV : 0;
}

static int dcn_check(int64_t B, int D, int L, const void* x0, int64_t ldx, const void* W,
                     const void* bias) {
  CTR_REQUIRE(B >= 0 && D >= 1 && D <= (1 << 24), "dcn_cross: bad sizes B=%lld D=%d",
              (long long)B, D);
  CTR_REQUIRE(L >= 1 && L <= kDcnMaxL, "dcn_cross: L=%d outside [1, %d]", L, kDcnMaxL);
  CTR_REQUIRE((x0 || B == 0) && W && bias, "dcn_cross: null x0 / W / bias");
  CTR_REQUIRE(ldx >= D, "dcn_cross: ldx %lld < D", (long long)ldx);
  return CTR_OK;
}

extern "C" int64_t ctr_dcn_cross_workspace_bytes(int64_t B, int D, int L) {
  if (B < 0 || D < 1 || L < 1 || L > kDcnMaxL) return 0;
  return (int64_t)kDcnMaxBlocks * ((int64_t)(L + 2) * D + kDcnTStride) * (int64_t)sizeof(float);
}

#define DCN_FWD_CASE(NVV)                                                                     \
  case NVV:                                                                                   \
    if (vec) {                                                                                \
      hipLaunchKernelGGL((dcn_forward_kernel<NVV, true>), grid, 256, 0, st, B, D, L, x0, ldx, \
                         W, bias, w_tail, s, xL, ldo, z);                                     \
    } else {                                                                                  \
      hipLaunchKernelGGL((dcn_forward_kernel<NVV, false>), grid, 256, 0, st, B, D, L, x0,     \
                         ldx, W, bias, w_tail, s, xL, ldo, z);                                \
    }                                                                                         \
    break

extern "C" int ctr_dcn_cross_forward(int64_t B, int D, int L, const float* x0, int64_t ldx,
                                     const float* W, const float* bias, const float* w_tail,
                                     float* s, float* xL, int64_t ldo, float* z,
                                     ctr_stream_t stream) {
  int rc = dcn_check(B, D, L, x0, ldx, W, bias);
  if (rc != CTR_OK) return rc;
  if (B == 0) return CTR_OK;  // nothing to write (empty outputs may be null)
  CTR_REQUIRE(s, "ctr_dcn_cross_forward: null s");
  CTR_REQUIRE(xL || z, "ctr_dcn_cross_forward: neither xL nor z requested");
  CTR_REQUIRE(!z || w_tail, "ctr_dcn_cross_forward: z needs w_tail");
  CTR_REQUIRE(!xL || ldo >= D, "ctr_dcn_cross_forward: ldo %lld < D", (long long)ldo);
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && dcn_al16(x0) && dcn_al16(W) && dcn_al16(bias) &&
                   (!w_tail || dcn_al16(w_tail)) && (!xL || (ldo % 4 == 0 && dcn_al16(xL)));
  hipStream_t st = as_stream(stream);
  const int nv = dcn_nv(D);
  if (nv == 0) {
    const unsigned grid = (unsigned)(B < 4096 ? B : 4096);
    if (vec) {
      hipLaunchKernelGGL(dcn_forward_generic<true>, grid, 256, 0, st, B, D, L, x0, ldx, W, bias,
                         w_tail, s, xL, ldo, z);
    } else {
      hipLaunchKernelGGL(dcn_forward_generic<false>, grid, 256, 0, st, B, D, L, x0, ldx, W, bias,
                         w_tail, s, xL, ldo, z);
    }
  } else {
    const int64_t nb = ceil_div(B, 4);
    const unsigned grid = (unsigned)(nb < 2048 ? nb : 2048);
    switch (nv) {
      DCN_FWD_CASE(1);
      DCN_FWD_CASE(2);
      DCN_FWD_CASE(4);
      DCN_FWD_CASE(7);
    }
  }
  CTR_LAUNCH_CHECK("ctr_dcn_cross_forward");
  return CTR_OK;
}

template <int NV>
static void dcn_launch_backward(bool vec, bool has_gl, unsigned grid, hipStream_t st, int64_t B,
                                int D, int L, const float* x0, int64_t ldx, const float* W,
                                const float* s, const float* gL, int64_t ldg, const float* gz,
                                const float* w_tail, float* dx0, int64_t ldd, float* pA,
                                float* pG, float* pT) {
  const size_t lds =
      ((size_t)(has_gl ? 2 : 1) * kDcnBwdRows * NV * 4 * kWave + kDcnBwdRows * kDcnCoef) *
      sizeof(float);
  const unsigned nt = kWave * kDcnBwdRows;
#define DCN_BWD_GO(V, G)                                                                       \
  hipLaunchKernelGGL((dcn_backward_kernel<NV, V, G>), grid, nt, lds, st, B, D, L, x0, ldx, W, \
                     s, gL, ldg, gz, w_tail, dx0, ldd, pA, pG, pT)
  if (vec && has_gl) {
    DCN_BWD_GO(true, true);
  } else if (vec) {
    DCN_BWD_GO(true, false);
  } else if (has_gl) {
    DCN_BWD_GO(false, true);
  } else {
    DCN_BWD_GO(false, false);
  }
#undef DCN_BWD_GO
}

extern "C" int ctr_dcn_cross_backward(int64_t B, int D, int L, const float* x0, int64_t ldx,
                                      const float* W, const float* bias, const float* s,
                                      const float* gL, int64_t ldg, const float* gz,
                                      const float* w_tail, float* dx0, int64_t ldd, float* dW,
                                      float* dbias, float* dw_tail, void* ws, int64_t ws_bytes,
                                      ctr_stream_t stream) {
  int rc = dcn_check(B, D, L, x0, ldx, W, bias);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(((s && dx0) || B == 0) && dW && dbias,
              "ctr_dcn_cross_backward: null s / dx0 / dW / dbias");
  CTR_REQUIRE(gL || gz || B == 0, "ctr_dcn_cross_backward: neither gL nor the rank-1 form given");
  CTR_REQUIRE((gz != nullptr) == (w_tail != nullptr) || B == 0,
              "ctr_dcn_cross_backward: gz and w_tail go together");
  CTR_REQUIRE(!dw_tail || w_tail, "ctr_dcn_cross_backward: dw_tail needs the rank-1 form");
  CTR_REQUIRE(ldd >= D && (!gL || ldg >= D), "ctr_dcn_cross_backward: ldd / ldg < D");
  const int64_t need = ctr_dcn_cross_workspace_bytes(B, D, L);
  if (!ws || ws_bytes < need || !dcn_al16(ws)) {
    set_error("ctr_dcn_cross_backward: workspace %lld < %lld bytes (or not 16-B aligned)",
              (long long)ws_bytes, (long long)need);
    return CTR_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  float* pA = static_cast<float*>(ws);
  float* pG = pA + (int64_t)kDcnMaxBlocks * (L + 1) * D;
  float* pT = pG + (int64_t)kDcnMaxBlocks * D;
  int nblk = 0;
  if (B > 0) {
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && ldd % 4 == 0 && dcn_al16(x0) && dcn_al16(W) &&
                     dcn_al16(dx0) && (!gL || (ldg % 4 == 0 && dcn_al16(gL))) &&
                     (!w_tail || dcn_al16(w_tail));
    int cap = kDcnMaxBlocks;
    if (const char* e = getenv("CTR_DCN_BLOCKS")) {  // A/B runs: fewer partial slabs
      const int v = atoi(e);
      if (v >= 1 && v < cap) cap = v;
    }
    const int nv = dcn_nv(D);
    // at least two passes per block once the batch allows: half the partial traffic
    const int64_t want = ceil_div(B, nv ? 2 * kDcnBwdRows : 2);
    nblk = (int)(want < cap ? want : cap);
    const unsigned grid = (unsigned)nblk;
    switch (nv) {
      case 0:
        if (vec) {
          hipLaunchKernelGGL(dcn_backward_generic<true>, grid, 256, 0, st, B, D, L, x0, ldx, W,
                             s, gL, ldg, gz, w_tail, dx0, ldd, pA, pG, pT);
        } else {
          hipLaunchKernelGGL(dcn_backward_generic<false>, grid, 256, 0, st, B, D, L, x0, ldx, W,
                             s, gL, ldg, gz, w_tail, dx0, ldd, pA, pG, pT);
        }
        break;
      case 1:
        dcn_launch_backward<1>(vec, gL != nullptr, grid, st, B, D, L, x0, ldx, W, s, gL, ldg, gz,
                               w_tail, dx0, ldd, pA, pG, pT);
        break;
      case 2:
        dcn_launch_backward<2>(vec, gL != nullptr, grid, st, B, D, L, x0, ldx, W, s, gL, ldg, gz,
                               w_tail, dx0, ldd, pA, pG, pT);
        break;
      case 4:
        dcn_launch_backward<4>(vec, gL != nullptr, grid, st, B, D, L, x0, ldx, W, s, gL, ldg, gz,
                               w_tail, dx0, ldd, pA, pG, pT);
        break;
      default:
        dcn_launch_backward<kDcnMaxNV>(vec, gL != nullptr, grid, st, B, D, L, x0, ldx, W, s, gL,
                                       ldg, gz, w_tail, dx0, ldd, pA, pG, pT);
        break;
    }
    CTR_LAUNCH_CHECK("ctr_dcn_cross_backward");
  }
  // nblk == 0 (B == 0): the sums are empty, the outputs zero
  hipLaunchKernelGGL(dcn_backward_finalize, dim3((unsigned)ceil_div(D, kWave), L + 2), 1024, 0,
                     st, D, L, nblk, pA, gL ? pG : nullptr, pT, W, bias, w_tail, dW, dbias,
                     dw_tail);
  CTR_LAUNCH_CHECK("ctr_dcn_cross_backward (finalize)");
  return CTR_OK;
}
