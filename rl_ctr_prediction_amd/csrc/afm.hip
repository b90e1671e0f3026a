// Attentional factorisation machine (AFM): the pairwise-attention pooling of p_model.AFM
// (reference src/models/p_model.py:438-486), forward and backward.
//
// Per example b with ids x[b, 0..F), pairs p = (i, j), i < j, in row-major order, P = F(F-1)/2:
//   e_f = E[x_f] [K];  q_p = e_i * e_j [K];  h_p = relu(W1 q_p + b1) [A];  s_p = <w2, h_p> + b2
//   a = softmax_p(s) (max-subtracted);  a'_p = a_p * m1[b, p];  o = sum_p a'_p q_p;  o' = o * m2
// Backward, from do':  do = do' * m2;  da_p = m1_p <do, q_p>;  c = sum_p a_p da_p;
//   ds_p = a_p (da_p - c);  dh_p = ds_p * w2 * [h_p > 0];  dq_p = W1^T dh_p + a'_p do;
//   de_i += dq_p * e_j, de_j += dq_p * e_i;  batch sums dW1 = sum dh_p (x) q_p, db1 = sum dh_p,
//   dw2 = sum ds_p h_p, db2 = sum ds_p.
// Neither the [B, P, K] pair tensor nor the [B, P, A] hidden layer nor the scores reach global
// memory: a block stages its example's F rows once in LDS and forms the pair products from
// them; the only activation the backward keeps is the softmax a [B, P].
//
// Forward. One block per example (blocks stride over the batch), one thread per pair: the
// thread holds q_p in registers (KR = 16 / 32 / 64 / 128 of them, zero past K) and walks the A
// hidden units, each two chains (even and odd columns) of plain fp32 FMAs whose W1 operand is
// the same in every lane (a wave-uniform load, no LDS traffic). Scores go to LDS, the softmax is two block
// reductions (butterfly per wave, waves in order), the pooling deals (pair group, column)
// items over the block and adds the groups in order. The block size follows P alone, so a row's
// result depends on nothing but the row.
//
// Backward. One 256-thread block per example, blocks striding over the batch:
//   A  (thread per pair)  da_p, then c by a block reduction, ds_p;
//   C  (thread per pair, q_p in registers as in the forward) the pre-activations again, kept as
//      one bit per (pair, hidden unit) in LDS;
//   D  (thread per 4 x 4 tile of [A, K], registers, kept across the block's examples)
//      T[a, k] += d_pa q_pk, S[a] += d_pa with d_pa = ds_p [h_pa > 0], pairs in order;
//   E  (thread per pair and 4 columns) dq_p = a'_p do + W1^T dh_p from the bits, once per pair,
//      added into the two slots' rows of an LDS accumulator: de_i += dq_p e_j, de_j += dq_p e_i.
//      The pairs go in the rounds of a round-robin schedule (no two pairs of a round share a
//      slot), a barrier between rounds: no atomics, a fixed order per slot.
// Each block writes its T, S and sum ds once, as one slab of the workspace; a second launch adds
// the slabs in block order and forms
//   dW1 = w2[a] T,  db1 = w2[a] S,  dw2[a] = b1[a] S[a] + sum_k W1[a, k] T[a, k],  db2 = sum ds
// (relu(x) = [x > 0] x, so dw2 needs no second pass over the pairs). No float atomics: the same
// bits every run.
#include <algorithm>

#include "ctr_common.h"

namespace ctr {

constexpr int kAfmMaxF = 64;
constexpr int kAfmMaxK = 128;
constexpr int kAfmMaxA = 128;
// forward block size, at most: the widest q leaves a thread 512 registers at 256 threads
__host__ __device__ constexpr int afm_fwd_threads(int KR) { return KR == 128 ? 256 : 512; }
constexpr int kAfmFwdMaxBlocks = 2048;
constexpr int kAfmBwdThreads = 256;
// backward blocks = partial slabs: the workspace ignores B. Mirrored by hand as
// hip_ops.AFM_BWD_MAX_BLOCKS (tests tie the two through ctr_afm_workspace_bytes): change both.
constexpr int kAfmMaxBlocks = 1024;
constexpr int kAfmTiles = 4;        // 4 x 4 tiles of [A, K] per backward thread: 1 or this many

__host__ __device__ inline int afm_pairs(int F) { return F * (F - 1) / 2; }
__host__ __device__ inline int afm_lde(int K) { return K | 1; }  // odd: rows on distinct banks
__host__ __device__ inline int afm_part(int nt, int K) { return nt > K ? nt : K; }

inline size_t afm_fwd_lds(int F, int K, int nt) {
  const int P = afm_pairs(F);
  return (size_t)F * 8 + ((size_t)F * afm_lde(K) + P + 16 + afm_part(nt, K)) * 4 + 2 * (size_t)P;
}
inline size_t afm_bwd_lds(int F, int K, int A) {
  const int P = afm_pairs(F), AW = (A + 31) / 32;
  return (size_t)F * 8 + (2 * (size_t)F * afm_lde(K) + 3 * (size_t)P + K + 16 + (size_t)P * AW) * 4 +
         2 * (size_t)P;
}

// sum / max over the block, the same value in every thread; waves added in order (red: 16)
__device__ __forceinline__ float afm_block_sum(float v, float* red) {
  v = wave_sum(v);
  const int nw = blockDim.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < nw; ++w) r += red[w];
  __syncthreads();
  return r;
}
__device__ __forceinline__ float afm_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  const int nw = blockDim.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < nw; ++w) r = fmaxf(r, red[w]);
  __syncthreads();
  return r;
}

// the (i, j) of every pair, row-major, once per block
__device__ __forceinline__ void afm_pair_table(int F, int P, uint8_t* pi, uint8_t* pj) {
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    int i = 0, rem = p;
    while (rem >= F - 1 - i) {
      rem -= F - 1 - i;
      ++i;
    }
    pi[p] = (uint8_t)i;
    pj[p] = (uint8_t)(i + 1 + rem);
  }
}

// the example's F rows into LDS (row stride lde); ids resolved once, by the first F threads
template <typename IdxT>
__device__ __forceinline__ void afm_stage(const IdxT* __restrict__ idx, int64_t b, int F, int K,
                                          int64_t V, const float* __restrict__ emb, bool vec,
                                          long long* rows, float* e, int lde, int32_t* err) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid < F) rows[tid] = (long long)load_row(idx, b * F + tid, V, err);
  __syncthreads();
  if (vec) {
    const int K4 = K >> 2;
    for (int t = tid; t < F * K4; t += nt) {
      const int f = t / K4, k = 4 * (t - f * K4);
      const float4 v = *reinterpret_cast<const float4*>(emb + rows[f] * K + k);
      float* d = e + f * lde + k;
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
  } else {
    for (int t = tid; t < F * K; t += nt) {
      const int f = t / K, k = t - f * K;
      e[f * lde + k] = emb[rows[f] * K + k];
    }
  }
  __syncthreads();
}

template <int KR, bool FULL>
__device__ __forceinline__ void afm_load_q(const float* ei, const float* ej, int K,
                                           float (&q)[KR]) {
#pragma unroll
  for (int u = 0; u < KR; ++u) q[u] = (FULL || u < K) ? ei[u] * ej[u] : 0.f;
}

// the pre-activation of hidden unit a: (b1 + the even columns' terms) + the odd columns' terms,
// each chain one FMA per term in column order (two chains: twice the FMAs in flight). a is
// uniform, so the W1 and b1 operands are the same in every lane.
template <int KR, bool FULL>
__device__ __forceinline__ float afm_hidden(const float* __restrict__ W1,
                                            const float* __restrict__ b1, int K, int a,
                                            const float (&q)[KR]) {
  const float* __restrict__ w = W1 + (int64_t)a * K;
  float h0 = b1[a], h1 = 0.f;
#pragma unroll
  for (int u = 0; u < KR; u += 2) {
    if (FULL || u < K) h0 = fmaf(w[u], q[u], h0);
    if (FULL || u + 1 < K) h1 = fmaf(w[u + 1], q[u + 1], h1);
  }
  return h0 + h1;
}

__device__ __forceinline__ float afm_keep(uint64_t seed, uint64_t ctr, uint32_t thr, float scale) {
  return hash_u32(seed, ctr) >= thr ? scale : 0.f;
}

// The dropout seed of a step: seed + t * the splitmix64 increment (mod 2^64), t = *step_ptr read
// once as an unsigned 32-bit value — a seed the host can compute, so the _step entry points at
// step t are the plain ones called with it. NULL: the seed itself. A captured graph replays
// the pointer, not the value: every replay draws the masks of its own step.
__device__ __forceinline__ uint64_t afm_step_seed(uint64_t seed, const int32_t* step_ptr) {
  return step_ptr ? seed + (uint64_t)(uint32_t)step_ptr[0] * 0x9E3779B97F4A7C15ull : seed;
}

// ------------------------------------------------------------------- forward ----------
template <typename IdxT, int KR, bool FULL>
__global__ __launch_bounds__(afm_fwd_threads(KR)) void afm_forward_kernel(
    const IdxT* __restrict__ idx, int64_t B, int F, int K, int A, int64_t V,
    const float* __restrict__ emb, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, int vec, int drop, uint32_t thr,
    float scale, uint64_t seed, const int32_t* __restrict__ step_ptr,
    float* __restrict__ pooled, int64_t ldp, float* __restrict__ attn, int32_t* err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char afm_lds[];
  seed = afm_step_seed(seed, step_ptr);
  const int P = afm_pairs(F), lde = afm_lde(K);
  const int tid = threadIdx.x, nt = blockDim.x;
  long long* rows = reinterpret_cast<long long*>(afm_lds);
  float* e = reinterpret_cast<float*>(rows + F);
  float* sc = e + F * lde;
  float* red = sc + P;
  float* part = red + 16;
  uint8_t* pi = reinterpret_cast<uint8_t*>(part + afm_part(nt, K));
  uint8_t* pj = pi + P;
  afm_pair_table(F, P, pi, pj);  // visible after afm_stage's barriers
  const float b2v = b2[0];
  const int G = nt >= K ? nt / K : 1;  // pooling: G groups of consecutive pairs
  const int chunk = (P + G - 1) / G;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    afm_stage(idx, b, F, K, V, emb, vec != 0, rows, e, lde, err);
    // scores
    for (int p = tid; p < P; p += nt) {
      float q[KR];
      afm_load_q<KR, FULL>(e + pi[p] * lde, e + pj[p] * lde, K, q);
      float s = b2v;
      for (int a = 0; a < A; ++a)
        s = fmaf(w2[a], fmaxf(afm_hidden<KR, FULL>(W1, b1, K, a, q), 0.f), s);
      sc[p] = s;
    }
    // softmax over the pairs; a thread touches its own pairs only
    float mx = -INFINITY;
    for (int p = tid; p < P; p += nt) mx = fmaxf(mx, sc[p]);
    mx = afm_block_max(mx, red);
    float sum = 0.f;
    for (int p = tid; p < P; p += nt) {
      const float ex = expf(sc[p] - mx);
      sc[p] = ex;
      sum += ex;
    }
    sum = afm_block_sum(sum, red);
    const uint64_t ctr0 = (uint64_t)b * (uint64_t)(P + K);
    for (int p = tid; p < P; p += nt) {
      float a = sc[p] / sum;
      if (attn) attn[b * P + p] = a;
      if (drop) a *= afm_keep(seed, ctr0 + (uint64_t)p, thr, scale);
      sc[p] = a;
    }
    __syncthreads();
    // pooling: part[g, k] = sum of a'_p q_pk over group g's pairs, then the groups in order
    for (int it = tid; it < G * K; it += nt) {
      const int g = it / K, k = it - g * K;
      const int p1 = (g + 1) * chunk < P ? (g + 1) * chunk : P;
      float acc = 0.f;
      for (int p = g * chunk; p < p1; ++p)
        acc = fmaf(sc[p], e[pi[p] * lde + k] * e[pj[p] * lde + k], acc);
      part[it] = acc;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      float o = part[k];
      for (int g = 1; g < G; ++g) o += part[g * K + k];
      if (drop) o *= afm_keep(seed, ctr0 + (uint64_t)(P + k), thr, scale);
      pooled[b * ldp + k] = o;
    }
    __syncthreads();  // e, sc and part are rewritten by the next example
  }
}

// ------------------------------------------------------------------ backward ----------
// Workspace: pT [kAfmMaxBlocks][A*K], pS [kAfmMaxBlocks][A], pD [kAfmMaxBlocks].
template <typename IdxT, int KR, bool FULL, int NT>
__global__ __launch_bounds__(kAfmBwdThreads) void afm_backward_kernel(
    const IdxT* __restrict__ idx, int64_t B, int F, int K, int A, int64_t V,
    const float* __restrict__ emb, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ w2, int vec_emb, int vec_w, int vec_out, int drop, uint32_t thr,
    float scale, uint64_t seed, const int32_t* __restrict__ step_ptr,
    const float* __restrict__ attn, const float* __restrict__ dpooled, int64_t ldg,
    float* __restrict__ dslot, float* __restrict__ pT, float* __restrict__ pS,
    float* __restrict__ pD, int32_t* err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char afm_lds[];
  seed = afm_step_seed(seed, step_ptr);
  const int P = afm_pairs(F), lde = afm_lde(K), AW = (A + 31) / 32;
  const int tid = threadIdx.x;
  constexpr int nt = kAfmBwdThreads;
  long long* rows = reinterpret_cast<long long*>(afm_lds);
  float* e = reinterpret_cast<float*>(rows + F);
  float* aL = e + F * lde;   // a_p
  float* apL = aL + P;       // a'_p = a_p m1_p
  float* dsL = apL + P;      // da_p, then ds_p
  float* dov = dsL + P;      // do [K]
  float* red = dov + K;
  float* deL = red + 16;     // the slots' gradients [F][lde]
  uint32_t* bits = reinterpret_cast<uint32_t*>(deL + F * lde);  // [P][AW]: h_pa > 0
  uint8_t* pi = reinterpret_cast<uint8_t*>(bits + (size_t)P * AW);
  uint8_t* pj = pi + P;
  afm_pair_table(F, P, pi, pj);
  // this thread's 4 x 4 tiles of [A, K]
  const int ntk = (K + 3) >> 2, ntiles = ((A + 3) >> 2) * ntk;
  int ta0[NT], tk0[NT];
  float accT[NT][16], accS[NT][4];
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    const int t = tid + nt * s;
    ta0[s] = 4 * (t / ntk);
    tk0[s] = 4 * (t % ntk);
#pragma unroll
    for (int r = 0; r < 16; ++r) accT[s][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) accS[s][r] = 0.f;
  }
  float dsum = 0.f;  // thread 0: sum of ds over the block's examples
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    afm_stage(idx, b, F, K, V, emb, vec_emb != 0, rows, e, lde, err);
    const uint64_t ctr0 = (uint64_t)b * (uint64_t)(P + K);
    for (int k = tid; k < K; k += nt) {
      float g = dpooled[b * ldg + k];
      if (drop) g *= afm_keep(seed, ctr0 + (uint64_t)(P + k), thr, scale);
      dov[k] = g;
    }
    __syncthreads();
    // A: da_p = m1_p <do, q_p>, c = sum_p a_p da_p, ds_p = a_p (da_p - c)
    float c = 0.f;
    for (int p = tid; p < P; p += nt) {
      const float* ei = e + pi[p] * lde;
      const float* ej = e + pj[p] * lde;
      float da = 0.f;
      for (int k = 0; k < K; ++k) da = fmaf(dov[k], ei[k] * ej[k], da);
      const float a = attn[b * P + p];
      const float m1 = drop ? afm_keep(seed, ctr0 + (uint64_t)p, thr, scale) : 1.f;
      da *= m1;
      aL[p] = a;
      apL[p] = a * m1;
      dsL[p] = da;
      c = fmaf(a, da, c);
    }
    c = afm_block_sum(c, red);
    float dl = 0.f;
    for (int p = tid; p < P; p += nt) {
      const float ds = aL[p] * (dsL[p] - c);
      dsL[p] = ds;
      dl += ds;
    }
    dl = afm_block_sum(dl, red);
    dsum += dl;
    // C: the ReLU's sign of every (pair, hidden unit), from the forward's own arithmetic
    for (int p = tid; p < P; p += nt) {
      float q[KR];
      afm_load_q<KR, FULL>(e + pi[p] * lde, e + pj[p] * lde, K, q);
      uint32_t word = 0;
      for (int a = 0; a < A; ++a) {
        if (afm_hidden<KR, FULL>(W1, b1, K, a, q) > 0.f) word |= 1u << (a & 31);
        if (((a + 1) & 31) == 0 || a + 1 == A) {
          bits[p * AW + (a >> 5)] = word;
          word = 0;
        }
      }
    }
    __syncthreads();
    // D: T[a, k] += d_pa q_pk, S[a] += d_pa over the pairs in order
    for (int p = 0; p < P; ++p) {
      const float dsp = dsL[p];
      const float* ei = e + pi[p] * lde;
      const float* ej = e + pj[p] * lde;
#pragma unroll
      for (int s = 0; s < NT; ++s) {
        if (tid + nt * s >= ntiles) continue;
        const uint32_t nib = (bits[p * AW + (ta0[s] >> 5)] >> (ta0[s] & 31)) & 15u;
        if (nib == 0) continue;
        float q[4], d[4];
#pragma unroll
        for (int cix = 0; cix < 4; ++cix) {
          const int k = tk0[s] + cix;
          q[cix] = k < K ? ei[k] * ej[k] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = ((nib >> r) & 1u) ? dsp : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int cix = 0; cix < 4; ++cix)
            accT[s][4 * r + cix] = fmaf(d[r], q[cix], accT[s][4 * r + cix]);
          accS[s][r] += d[r];
        }
      }
    }
    // E: de_i += dq_p e_j and de_j += dq_p e_i, dq_p = a'_p do + W1^T dh_p evaluated once per
    // pair. The pairs are taken in the n - 1 rounds of a round-robin schedule over n = F (or
    // F + 1: a bye) slots: no two pairs of a round share a slot, so a round's items own their
    // rows of deL, and a slot's F - 1 contributions arrive in round order.
    for (int t = tid; t < F * lde; t += nt) deL[t] = 0.f;
    const int nrr = (F + 1) & ~1;
    for (int r = 0; r < nrr - 1; ++r) {
      __syncthreads();
      for (int it = tid; it < (nrr >> 1) * ntk; it += nt) {
        const int m = it / ntk, k0 = 4 * (it - m * ntk);
        const int i = m == 0 ? nrr - 1 : (r + m) % (nrr - 1);
        const int j = m == 0 ? r : (r + nrr - 1 - m) % (nrr - 1);
        if (i >= F || j >= F) continue;  // the bye of an odd F
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int p = lo * (2 * F - lo - 1) / 2 + (hi - lo - 1);
        const float dsp = dsL[p], ap = apL[p];
        float dq[4];
#pragma unroll
        for (int cix = 0; cix < 4; ++cix) dq[cix] = k0 + cix < K ? ap * dov[k0 + cix] : 0.f;
        for (int w = 0; w < AW; ++w) {
          const uint32_t word = bits[p * AW + w];
          const int a1 = 32 * w + 32 < A ? 32 * w + 32 : A;
          for (int a = 32 * w; a < a1; ++a) {
            const float dh = ((word >> (a & 31)) & 1u) ? dsp * w2[a] : 0.f;
            const float* wr = W1 + (int64_t)a * K + k0;
            if (vec_w) {
              const float4 wv = *reinterpret_cast<const float4*>(wr);
              dq[0] = fmaf(wv.x, dh, dq[0]);
              dq[1] = fmaf(wv.y, dh, dq[1]);
              dq[2] = fmaf(wv.z, dh, dq[2]);
              dq[3] = fmaf(wv.w, dh, dq[3]);
            } else {
#pragma unroll
              for (int cix = 0; cix < 4; ++cix)
                if (k0 + cix < K) dq[cix] = fmaf(wr[cix], dh, dq[cix]);
            }
          }
        }
        const float* ei = e + i * lde + k0;
        const float* ej = e + j * lde + k0;
        float* di = deL + i * lde + k0;
        float* dj = deL + j * lde + k0;
#pragma unroll
        for (int cix = 0; cix < 4; ++cix) {
          if (k0 + cix < K) {
            di[cix] = fmaf(dq[cix], ej[cix], di[cix]);
            dj[cix] = fmaf(dq[cix], ei[cix], dj[cix]);
          }
        }
      }
    }
    __syncthreads();
    for (int it = tid; it < F * ntk; it += nt) {
      const int i = it / ntk, k0 = 4 * (it - i * ntk);
      const float* di = deL + i * lde + k0;
      float* o = dslot + (b * F + i) * K + k0;
      if (vec_out) {
        *reinterpret_cast<float4*>(o) = make_float4(di[0], di[1], di[2], di[3]);
      } else {
#pragma unroll
        for (int cix = 0; cix < 4; ++cix)
          if (k0 + cix < K) o[cix] = di[cix];
      }
    }
    __syncthreads();  // the LDS arrays are rewritten by the next example
  }
  float* Tb = pT + (int64_t)blockIdx.x * A * K;
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    if (tid + nt * s >= ntiles) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = ta0[s] + r;
      if (a >= A) continue;
#pragma unroll
      for (int cix = 0; cix < 4; ++cix)
        if (tk0[s] + cix < K) Tb[(int64_t)a * K + tk0[s] + cix] = accT[s][4 * r + cix];
      if (tk0[s] == 0) pS[(int64_t)blockIdx.x * A + a] = accS[s][r];
    }
  }
  if (tid == 0) pD[blockIdx.x] = dsum;
}

// The slabs in block order -> dW1, db1, dw2, db2. One block per hidden unit a, thread k.
__global__ __launch_bounds__(kAfmMaxK) void afm_backward_finalize(
    int K, int A, int nblk, const float* __restrict__ pT, const float* __restrict__ pS,
    const float* __restrict__ pD, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ w2, float* __restrict__ dW1, float* __restrict__ db1,
    float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ float prod[kAfmMaxK];
  const int a = blockIdx.x, k = threadIdx.x;
  if (k < K) {
    float t = 0.f;
    for (int n = 0; n < nblk; ++n) t += pT[((int64_t)n * A + a) * K + k];
    dW1[(int64_t)a * K + k] = w2[a] * t;
    prod[k] = W1[(int64_t)a * K + k] * t;
  }
  __syncthreads();
  if (k != 0) return;
  float s = 0.f;
  for (int n = 0; n < nblk; ++n) s += pS[(int64_t)n * A + a];
  db1[a] = w2[a] * s;
  float v = b1[a] * s;
  for (int kk = 0; kk < K; ++kk) v += prod[kk];
  dw2[a] = v;
  if (a == 0) {
    float d = 0.f;
    for (int n = 0; n < nblk; ++n) d += pD[n];
    db2[0] = d;
  }
}

}  // namespace ctr

using namespace ctr;

static bool afm_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int afm_check(const char* who, const void* idx, int idx_type, int64_t B, int F, int K,
                     int A, int64_t V, const void* emb, const void* W1, const void* b1,
                     const void* w2, const void* b2, float drop_p) {
  CTR_REQUIRE(B >= 0 && V >= 1, "%s: bad sizes B=%lld V=%lld", who, (long long)B, (long long)V);
  CTR_REQUIRE(F >= 2 && F <= kAfmMaxF, "%s: F=%d outside [2, %d]", who, F, kAfmMaxF);
  CTR_REQUIRE(K >= 1 && K <= kAfmMaxK, "%s: K=%d outside [1, %d]", who, K, kAfmMaxK);
  CTR_REQUIRE(A >= 1 && A <= kAfmMaxA, "%s: A=%d outside [1, %d]", who, A, kAfmMaxA);
  CTR_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", who,
              (double)drop_p);
  CTR_REQUIRE(idx_type == CTR_IDX_I32 || idx_type == CTR_IDX_I64, "%s: bad idx_type %d", who,
              idx_type);
  CTR_REQUIRE(idx || B == 0, "%s: null idx", who);
  CTR_REQUIRE(emb, "%s: null emb", who);
  CTR_REQUIRE(W1 && b1 && w2 && b2, "%s: null W1 / b1 / w2 / b2", who);
  return CTR_OK;
}

static void afm_drop(float drop_p, uint32_t* thr, float* scale) {
  *thr = (uint32_t)std::min<double>((double)drop_p * 4294967296.0, 4294967295.0);
  *scale = (float)(1.0 / (1.0 - (double)drop_p));
}

// K -> the register width KR of a pair thread's q, as a template argument
template <typename Fn>
static void afm_dispatch_kr(int K, Fn&& f) {
  if (K <= 16)
    f(std::integral_constant<int, 16>{});
  else if (K <= 32)
    f(std::integral_constant<int, 32>{});
  else if (K <= 64)
    f(std::integral_constant<int, 64>{});
  else
    f(std::integral_constant<int, 128>{});
}

extern "C" int64_t ctr_afm_workspace_bytes(int64_t B, int F, int K, int A) {
  if (B < 0 || F < 2 || F > kAfmMaxF || K < 1 || K > kAfmMaxK || A < 1 || A > kAfmMaxA) return 0;
  return align_up((int64_t)kAfmMaxBlocks * ((int64_t)A * K + A + 1) * (int64_t)sizeof(float), 16);
}

static int afm_forward_impl(const char* who, const void* idx, int idx_type, int64_t B, int F,
                            int K, int A, int64_t V, const float* emb, const float* W1,
                            const float* b1, const float* w2, const float* b2, float drop_p,
                            uint64_t seed, const int32_t* step_ptr, float* pooled, int64_t ldp,
                            float* attn, int32_t* err_flag, ctr_stream_t stream) {
  int rc = afm_check(who, idx, idx_type, B, F, K, A, V, emb, W1, b1, w2, b2, drop_p);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(pooled || B == 0, "%s: null pooled", who);
  CTR_REQUIRE(ldp >= K, "%s: ldp %lld < K = %d", who, (long long)ldp, K);
  if (B == 0) return CTR_OK;
  const int P = afm_pairs(F);
  const int64_t want = ceil_div(P, kWave) * kWave;  // one thread per pair, whole waves
  const int cap = afm_fwd_threads(K > 64 ? 128 : 64);
  const unsigned nt = (unsigned)(want < cap ? want : cap);
  const unsigned grid = (unsigned)(B < kAfmFwdMaxBlocks ? B : kAfmFwdMaxBlocks);
  const size_t lds = afm_fwd_lds(F, K, (int)nt);
  const int vec = K % 4 == 0 && afm_al16(emb);
  const int drop = drop_p > 0.f;
  uint32_t thr;
  float scale;
  afm_drop(drop_p, &thr, &scale);
  hipStream_t st = as_stream(stream);
  afm_dispatch_kr(K, [&](auto w) {
    constexpr int KR = decltype(w)::value;
    dispatch_bool(K == KR, [&](auto fl) {
      constexpr bool FULL = decltype(fl)::value;
      dispatch_bool(idx_type == CTR_IDX_I64, [&](auto i64) {
        using IdxT = std::conditional_t<decltype(i64)::value, int64_t, int32_t>;
        auto kernel = afm_forward_kernel<IdxT, KR, FULL>;
        rc = allow_lds(kernel, lds);
        if (rc != CTR_OK) return;
        hipLaunchKernelGGL(kernel, grid, nt, lds, st, static_cast<const IdxT*>(idx), B, F, K, A,
                           V, emb, W1, b1, w2, b2, vec, drop, thr, scale, seed, step_ptr, pooled,
                           ldp, attn, err_flag);
      });
    });
  });
  if (rc != CTR_OK) return rc;
  CTR_LAUNCH_CHECK(who);
  return CTR_OK;
}

extern "C" int ctr_afm_forward(const void* idx, int idx_type, int64_t B, int F, int K, int A,
                               int64_t V, const float* emb, const float* W1, const float* b1,
                               const float* w2, const float* b2, float drop_p, uint64_t seed,
                               float* pooled, int64_t ldp, float* attn, int32_t* err_flag,
                               ctr_stream_t stream) {
  return afm_forward_impl("ctr_afm_forward", idx, idx_type, B, F, K, A, V, emb, W1, b1, w2, b2,
                          drop_p, seed, nullptr, pooled, ldp, attn, err_flag, stream);
}

extern "C" int ctr_afm_forward_step(const void* idx, int idx_type, int64_t B, int F, int K,
                                    int A, int64_t V, const float* emb, const float* W1,
                                    const float* b1, const float* w2, const float* b2,
                                    float drop_p, uint64_t seed, const int32_t* step_ptr,
                                    float* pooled, int64_t ldp, float* attn, int32_t* err_flag,
                                    ctr_stream_t stream) {
  return afm_forward_impl("ctr_afm_forward_step", idx, idx_type, B, F, K, A, V, emb, W1, b1, w2,
                          b2, drop_p, seed, step_ptr, pooled, ldp, attn, err_flag, stream);
}

static int afm_backward_impl(const char* who, const void* idx, int idx_type, int64_t B, int F,
                             int K, int A, int64_t V, const float* emb, const float* W1,
                             const float* b1, const float* w2, const float* b2, float drop_p,
                             uint64_t seed, const int32_t* step_ptr, const float* attn,
                             const float* dpooled, int64_t ldg, float* dslot, float* dW1,
                             float* db1, float* dw2, float* db2, void* ws, int64_t ws_bytes,
                             int32_t* err_flag, ctr_stream_t stream) {
  int rc = afm_check(who, idx, idx_type, B, F, K, A, V, emb, W1, b1, w2, b2, drop_p);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE((attn && dpooled && dslot) || B == 0, "%s: null attn / dpooled / dslot", who);
  CTR_REQUIRE(dW1 && db1 && dw2 && db2, "%s: null dW1 / db1 / dw2 / db2", who);
  CTR_REQUIRE(ldg >= K, "%s: ldg %lld < K = %d", who, (long long)ldg, K);
  const int64_t need = ctr_afm_workspace_bytes(B, F, K, A);
  CTR_REQUIRE(ws && ws_bytes >= need, "%s: workspace %lld < %lld bytes", who,
              (long long)ws_bytes, (long long)need);
  hipStream_t st = as_stream(stream);
  float* pT = static_cast<float*>(ws);
  float* pS = pT + (int64_t)kAfmMaxBlocks * A * K;
  float* pD = pS + (int64_t)kAfmMaxBlocks * A;
  int nblk = 0;
  if (B > 0) {
    nblk = (int)(B < kAfmMaxBlocks ? B : kAfmMaxBlocks);
    const size_t lds = afm_bwd_lds(F, K, A);
    const int vec_emb = K % 4 == 0 && afm_al16(emb);
    const int vec_w = K % 4 == 0 && afm_al16(W1);
    const int vec_out = K % 4 == 0 && afm_al16(dslot);
    const int drop = drop_p > 0.f;
    uint32_t thr;
    float scale;
    afm_drop(drop_p, &thr, &scale);
    // one 4 x 4 tile of [A, K] per thread where that covers the matrix (A = K = 64 does)
    const bool one_tile = ((A + 3) / 4) * ((K + 3) / 4) <= kAfmBwdThreads;
    afm_dispatch_kr(K, [&](auto w) {
      constexpr int KR = decltype(w)::value;
      dispatch_bool(K == KR, [&](auto fl) {
        constexpr bool FULL = decltype(fl)::value;
        dispatch_bool(one_tile, [&](auto ot) {
          constexpr int NT = decltype(ot)::value ? 1 : kAfmTiles;
          dispatch_bool(idx_type == CTR_IDX_I64, [&](auto i64) {
            using IdxT = std::conditional_t<decltype(i64)::value, int64_t, int32_t>;
            auto kernel = afm_backward_kernel<IdxT, KR, FULL, NT>;
            rc = allow_lds(kernel, lds);
            if (rc != CTR_OK) return;
            hipLaunchKernelGGL(kernel, (unsigned)nblk, kAfmBwdThreads, lds, st,
                               static_cast<const IdxT*>(idx), B, F, K, A, V, emb, W1, b1, w2,
                               vec_emb, vec_w, vec_out, drop, thr, scale, seed, step_ptr, attn,
                               dpooled, ldg, dslot, pT, pS, pD, err_flag);
          });
        });
      });
    });
    if (rc != CTR_OK) return rc;
    CTR_LAUNCH_CHECK(who);
  }
  // nblk == 0 (B == 0): the sums are empty, the outputs zero
  hipLaunchKernelGGL(afm_backward_finalize, (unsigned)A, kAfmMaxK, 0, st, K, A, nblk, pT, pS, pD,
                     W1, b1, w2, dW1, db1, dw2, db2);
  CTR_LAUNCH_CHECK("ctr_afm_backward (finalize)");
  return CTR_OK;
}

extern "C" int ctr_afm_backward(const void* idx, int idx_type, int64_t B, int F, int K, int A,
                                int64_t V, const float* emb, const float* W1, const float* b1,
                                const float* w2, const float* b2, float drop_p, uint64_t seed,
                                const float* attn, const float* dpooled, int64_t ldg,
                                float* dslot, float* dW1, float* db1, float* dw2, float* db2,
                                void* ws, int64_t ws_bytes, int32_t* err_flag,
                                ctr_stream_t stream) {
  return afm_backward_impl("ctr_afm_backward", idx, idx_type, B, F, K, A, V, emb, W1, b1, w2, b2,
                           drop_p, seed, nullptr, attn, dpooled, ldg, dslot, dW1, db1, dw2, db2,
                           ws, ws_bytes, err_flag, stream);
}

extern "C" int ctr_afm_backward_step(const void* idx, int idx_type, int64_t B, int F, int K,
                                     int A, int64_t V, const float* emb, const float* W1,
                                     const float* b1, const float* w2, const float* b2,
                                     float drop_p, uint64_t seed, const int32_t* step_ptr,
                                     const float* attn, const float* dpooled, int64_t ldg,
                                     float* dslot, float* dW1, float* db1, float* dw2,
                                     float* db2, void* ws, int64_t ws_bytes, int32_t* err_flag,
                                     ctr_stream_t stream) {
  return afm_backward_impl("ctr_afm_backward_step", idx, idx_type, B, F, K, A, V, emb, W1, b1,
                           w2, b2, drop_p, seed, step_ptr, attn, dpooled, ldg, dslot, dW1, db1,
                           dw2, db2, ws, ws_bytes, err_flag, stream);
}
