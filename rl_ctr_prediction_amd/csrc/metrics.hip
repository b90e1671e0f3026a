// Evaluation metrics on the device: exact ROC AUC, BCE loss and reward totals
// of a stream of batches, with no host read until the epoch's single read of the state block.
//
//   append  one launch per batch (n <= kAppSingleMax; two above): example i of the batch
//           becomes the 64-bit record (key << 1) | label at records[offset + i]. key is the
//           order-preserving uint32 image of the bits of p + 0.0f (-0.0 becomes +0.0, on the
//           integer side), so that -0.0 and +0.0 tie (sklearn ties them). In the same pass the BCE
//           -(y max(log p, -100) + (1-y) max(log(1-p), -100)) is summed in fp64 (log in
//           double of the fp32 p; y in {0, 1} selects one of the two terms, the other is an
//           exact 0), and so are the rewards. Every sum has an order fixed by n alone: a
//           thread adds its strided elements in order, a butterfly adds the lanes, one thread
//           adds the waves in order; blocks leave partials in block order and one block adds
//           them in a fixed order. No floating-point atomics: the same inputs give the same
//           bits. A NaN prediction, a label other than 0/1 and (when the loss is asked for) a
//           prediction outside [0, 1] raise a bit of the state's flag word (an integer OR) and
//           add nothing to the loss; the record is still written, inside [offset, offset + n).
//   sort    the count records by their low 33 bits: a stable LSD radix sort, digits of 9, 8, 8
//           and 8 bits, built like the flat sparse plan (sparse_plan.hip): per pass one launch
//           for the per-tile LDS histograms (integer atomics) and one in which every block
//           scans the tile histograms itself, ranks its records stably with wave ballots and
//           scatters. Key-only: the label rides in bit 0, so inside a run of equal keys the
//           negatives come first. Four passes: the sorted records end in the record buffer.
//   reduce  P, N and U2 = sum over positives of (2 x negatives strictly below + negatives
//           tied). With NP(i) = negatives at positions < i and S(i) = NP(start of i's run of
//           equal keys), a positive at i adds NP(i) + S(i). NP is non-decreasing, so S(i) is
//           the MAXIMUM of NP(s) over the run starts s <= i: a max-scan, inside a tile and over
//           the tiles before it (a run may start in an earlier tile and cover whole tiles).
//           Launch 1 leaves per tile its negatives and NP-within-the-tile at its last run
//           start; launch 2 scans those for its tile's bases and sums in uint64 (integer
//           atomics for the three totals: order-free). Exact for count < 2^31.
// AUC = U2 / (2 P N) is one double division on the host.
#include "ctr_common.h"

namespace ctr {

constexpr int kMetThreads = 256;
constexpr int kMetWaves = kMetThreads / kWave;
constexpr int kMetIPT = 16;
constexpr int kMetTile = kMetThreads * kMetIPT;  // records per sort tile and per reduce tile
constexpr int kAppThreads = 1024;
constexpr int kAppWaves = kAppThreads / kWave;
constexpr int kAppChunk = 4096;        // examples per block of the two-launch append
constexpr int kAppSingleMax = 16384;   // up to here one block appends and combines
constexpr int kMetFirstBits = 9, kMetBits = 8, kMetPasses = 4;  // 9 + 8 + 8 + 8 = 33 bits

struct MetricsState {  // the 128-byte state block of include/ctr_hip.h
  unsigned long long u2, pos, neg;
  double loss_sum, nll_sum, reward_sum;
  long long batches, loss_count;
  int32_t flags;
  int32_t reserved[15];
};
static_assert(sizeof(MetricsState) == CTR_METRICS_STATE_BYTES, "state block layout");

struct AppendArgs {
  const float* pred;
  int64_t stride;
  const void* labels;
  const float* rewards;
  int64_t n;
  uint64_t* rec;  // records + offset
  int with_loss;
  double* partials;  // [blocks][2]
  MetricsState* state;
};

__device__ __forceinline__ void metrics_commit(const AppendArgs& a, double loss, double reward) {
  if (a.with_loss) {
    a.state->loss_sum += loss / (double)a.n;
    a.state->nll_sum += loss;
    a.state->batches += 1;
    a.state->loss_count += a.n;
  }
  if (a.rewards) a.state->reward_sum += reward;
}

template <typename LT, bool SINGLE>
__global__ __launch_bounds__(kAppThreads) void metrics_append_kernel(AppendArgs a) {
  __shared__ double s_l[kAppWaves], s_r[kAppWaves];
  const LT* lab = static_cast<const LT*>(a.labels);
  const int64_t lo = SINGLE ? 0 : (int64_t)blockIdx.x * kAppChunk;
  const int64_t hi = SINGLE ? a.n : min(a.n, lo + (int64_t)kAppChunk);
  double ls = 0.0, rs = 0.0;
  int32_t fl = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kAppThreads) {
    const float p = a.pred[i * a.stride];
    const LT yv = lab[i];
    const bool one = yv == (LT)1, zero = yv == (LT)0;
    const bool nan = p != p;
    if (!(one || zero)) fl |= CTR_METRICS_FLAG_LABEL;
    if (nan) fl |= CTR_METRICS_FLAG_NAN;
    // the bits of p + 0.0f (-0.0 + 0.0 = +0.0: the zeros tie), taken on the integer side so
    // that no floating-point mode (denormal flushing) can touch the other values
    uint32_t b = __float_as_uint(p);
    b = b == 0x80000000u ? 0u : b;
    const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    a.rec[i] = ((uint64_t)key << 1) | (one ? 1ull : 0ull);
    if (a.with_loss && !nan) {
      if ((b & 0x80000000u) || !(p <= 1.0f)) {  // below zero (denormals included) or above one
        fl |= CTR_METRICS_FLAG_RANGE;
      } else if (one || zero) {
        const double pd = (double)p;
        ls -= fmax(log(one ? pd : 1.0 - pd), -100.0);
      }
    }
    if (a.rewards) rs += (double)a.rewards[i];
  }
  if (fl) atomicOr(&a.state->flags, fl);
  ls = wave_sum_f64(ls);
  rs = wave_sum_f64(rs);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  if (lane == 0) {
    s_l[w] = ls;
    s_r[w] = rs;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double L = 0.0, R = 0.0;
    for (int j = 0; j < kAppWaves; ++j) {
      L += s_l[j];
      R += s_r[j];
    }
    if (SINGLE) {
      metrics_commit(a, L, R);
    } else {
      a.partials[2 * (int64_t)blockIdx.x] = L;
      a.partials[2 * (int64_t)blockIdx.x + 1] = R;
    }
  }
}

// the blocks' partials, added in an order fixed by their number: thread t adds blocks t,
// t + 256, ... in order, then the lanes, then the waves
__global__ __launch_bounds__(kMetThreads) void metrics_combine_kernel(AppendArgs a, int nb) {
  __shared__ double s_l[kMetWaves], s_r[kMetWaves];
  double ls = 0.0, rs = 0.0;
  for (int j = threadIdx.x; j < nb; j += kMetThreads) {
    ls += a.partials[2 * (int64_t)j];
    rs += a.partials[2 * (int64_t)j + 1];
  }
  ls = wave_sum_f64(ls);
  rs = wave_sum_f64(rs);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_l[threadIdx.x / kWave] = ls;
    s_r[threadIdx.x / kWave] = rs;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double L = 0.0, R = 0.0;
    for (int j = 0; j < kMetWaves; ++j) {
      L += s_l[j];
      R += s_r[j];
    }
    metrics_commit(a, L, R);
  }
}

// ------------------------------------------------------------------- the sort ---------
struct MetSortPass {
  const uint64_t* in;
  uint64_t* out;
  int32_t* hist;  // [n_tiles][bins]
  int64_t count;
  int n_tiles;
  int shift;
};

template <int BITS>
__global__ __launch_bounds__(kMetThreads) void metrics_hist_kernel(MetSortPass a) {
  constexpr int R = 1 << BITS;
  __shared__ int32_t h[R];
  const int t = threadIdx.x;
  for (int d = t; d < R; d += kMetThreads) h[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kMetTile;
#pragma unroll
  for (int i = 0; i < kMetIPT; ++i) {
    const int64_t e = base + i * kMetThreads + t;
    if (e < a.count) atomicAdd(&h[(uint32_t)(a.in[e] >> a.shift) & (R - 1)], 1);
  }
  __syncthreads();
  for (int d = t; d < R; d += kMetThreads) a.hist[(int64_t)blockIdx.x * R + d] = h[d];
}

// exclusive sum scan of one value per thread over the 256-thread block; *total = the sum
__device__ __forceinline__ int32_t met_exscan(int32_t v, int32_t* s_w, int32_t* total) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  int32_t x = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int32_t y = __shfl_up(x, o, kWave);
    if (lane >= o) x += y;
  }
  if (lane == kWave - 1) s_w[w] = x;
  __syncthreads();
  int32_t off = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < kMetWaves; ++j) {
    off += j < w ? s_w[j] : 0;
    tot += s_w[j];
  }
  __syncthreads();
  if (total) *total = tot;
  return off + x - v;
}

// One pass over one tile, as radix_scatter_kernel of sparse_plan.hip on 64-bit records with no
// value: the block scans the tile histograms for its global digit bases (thread t owns the
// DPT digits [t*DPT, (t+1)*DPT)), ranks its records stably with wave ballots (the tile is
// striped, item i of thread t = tile + i*256 + t, so (item, wave, lane) order is input order),
// G item rows per pair of barriers, and scatters.
template <int BITS>
__global__ __launch_bounds__(kMetThreads) void metrics_scatter_kernel(MetSortPass a) {
  constexpr int R = 1 << BITS, DPT = R / kMetThreads, IPT = kMetIPT;
  constexpr int G = R <= 256 ? 4 : 2;  // item rows ranked together (2 x 16 KB of counts)
  static_assert(DPT >= 1 && IPT % G == 0, "digit ownership / ranking group");
  __shared__ int32_t s_base[R];
  __shared__ int32_t s_run[R];
  __shared__ int32_t s_cnt[G][kMetWaves][R];
  __shared__ int32_t s_pre[G][kMetWaves][R];
  __shared__ int32_t s_wtot[kMetWaves];
  const int t = threadIdx.x;
  const int lane = t & (kWave - 1), w = t / kWave;
  const int tile = blockIdx.x;
  const int64_t base = (int64_t)tile * kMetTile;
  uint64_t key[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int64_t e = base + i * kMetThreads + t;
    key[i] = e < a.count ? a.in[e] : 0ull;
  }

  int32_t tot[DPT], before[DPT];
#pragma unroll
  for (int k = 0; k < DPT; ++k) tot[k] = before[k] = 0;
  {
    const int32_t* hcol = a.hist + t * DPT;
    constexpr int U = 8;  // tile rows loaded together
    for (int j0 = 0; j0 < a.n_tiles; j0 += U) {
      int32_t hv[U][DPT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < DPT; ++k)
          hv[u][k] = j0 + u < a.n_tiles ? hcol[(int64_t)(j0 + u) * R + k] : 0;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
          tot[k] += hv[u][k];
          before[k] += j0 + u < tile ? hv[u][k] : 0;
        }
    }
  }
  int32_t mine = 0;
#pragma unroll
  for (int k = 0; k < DPT; ++k) mine += tot[k];
  int32_t start = met_exscan(mine, s_wtot, nullptr);
#pragma unroll
  for (int k = 0; k < DPT; ++k) {
    s_base[t * DPT + k] = start + before[k];
    s_run[t * DPT + k] = 0;
    start += tot[k];
  }
  for (int d = t; d < R; d += kMetThreads)
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
      for (int j = 0; j < kMetWaves; ++j) s_cnt[i][j][d] = 0;
  __syncthreads();

  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
  int32_t pos[IPT];
#pragma unroll
  for (int g0 = 0; g0 < IPT; g0 += G) {
    int rank[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int64_t e = base + (g0 + i) * kMetThreads + t;
      const bool ok = e < a.count;
      const uint32_t d = (uint32_t)(key[g0 + i] >> a.shift) & (R - 1);
      uint64_t peers = __ballot(ok);
#pragma unroll
      for (int b = 0; b < BITS; ++b) {
        const uint64_t m = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? m : ~m;
      }
      rank[i] = __popcll(peers & lt);
      if (ok && rank[i] == 0) s_cnt[i][w][d] = __popcll(peers);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int dd = t * DPT + k;
      int32_t run = s_run[dd];
#pragma unroll
      for (int i = 0; i < G; ++i)
#pragma unroll
        for (int j = 0; j < kMetWaves; ++j) {
          const int32_t c = s_cnt[i][j][dd];
          s_pre[i][j][dd] = run;
          s_cnt[i][j][dd] = 0;
          run += c;
        }
      s_run[dd] = run;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int64_t e = base + (g0 + i) * kMetThreads + t;
      const uint32_t d = (uint32_t)(key[g0 + i] >> a.shift) & (R - 1);
      pos[g0 + i] = e < a.count ? s_base[d] + s_pre[i][w][d] + rank[i] : -1;
    }
  }
#pragma unroll
  for (int i = 0; i < IPT; ++i)
    if (pos[i] >= 0 && pos[i] < a.count) a.out[pos[i]] = key[i];
}

// ------------------------------------------------------------------ the reduce --------
// Thread t owns the IPT consecutive sorted positions from tile*kMetTile + t*IPT on.
struct TileItems {
  bool live[kMetIPT], neg[kMetIPT], start[kMetIPT];
  int32_t cnt;  // negatives among them
};

__device__ __forceinline__ void met_load_items(const uint64_t* __restrict__ rec, int64_t count,
                                               int64_t s0, TileItems& it) {
  uint64_t prev = (s0 > 0 && s0 - 1 < count) ? rec[s0 - 1] >> 1 : ~0ull;
  it.cnt = 0;
#pragma unroll
  for (int i = 0; i < kMetIPT; ++i) {
    const int64_t s = s0 + i;
    it.live[i] = s < count;
    const uint64_t r = it.live[i] ? rec[s] : 0ull;
    const uint64_t k = r >> 1;
    it.neg[i] = it.live[i] && !(r & 1ull);
    it.start[i] = it.live[i] && (s == 0 || k != prev);
    prev = k;
    it.cnt += it.neg[i] ? 1 : 0;
  }
}

__device__ __forceinline__ int32_t met_block_max(int32_t v, int32_t* s_w) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = v;
  __syncthreads();
  int32_t r = s_w[0];
#pragma unroll
  for (int j = 1; j < kMetWaves; ++j) r = max(r, s_w[j]);
  __syncthreads();
  return r;
}

// exclusive max scan over the block (identity -1)
__device__ __forceinline__ int32_t met_exmaxscan(int32_t v, int32_t* s_w) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  int32_t x = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int32_t y = __shfl_up(x, o, kWave);
    if (lane >= o) x = max(x, y);
  }
  if (lane == kWave - 1) s_w[w] = x;
  __syncthreads();
  int32_t off = -1;
#pragma unroll
  for (int j = 0; j < kMetWaves; ++j) off = j < w ? max(off, s_w[j]) : off;
  __syncthreads();
  const int32_t up = __shfl_up(x, 1, kWave);
  return lane == 0 ? off : max(off, up);
}

// per tile: its negatives, and the negatives of the tile before its last run start (-1: no
// run starts in this tile)
__global__ __launch_bounds__(kMetThreads) void metrics_tile_count_kernel(
    const uint64_t* __restrict__ rec, int64_t count, int32_t* __restrict__ tile_neg,
    int32_t* __restrict__ tile_ls) {
  __shared__ int32_t s_w[kMetWaves];
  TileItems it;
  met_load_items(rec, count, (int64_t)blockIdx.x * kMetTile + (int64_t)threadIdx.x * kMetIPT, it);
  int32_t total;
  int32_t run = met_exscan(it.cnt, s_w, &total);
  int32_t last = -1;
#pragma unroll
  for (int i = 0; i < kMetIPT; ++i) {
    if (it.start[i]) last = run;
    run += it.neg[i] ? 1 : 0;
  }
  last = met_block_max(last, s_w);
  if (threadIdx.x == 0) {
    tile_neg[blockIdx.x] = total;
    tile_ls[blockIdx.x] = last;
  }
}

__global__ __launch_bounds__(kMetThreads) void metrics_reduce_kernel(
    const uint64_t* __restrict__ rec, int64_t count, const int32_t* __restrict__ tile_neg,
    const int32_t* __restrict__ tile_ls, MetricsState* state) {
  __shared__ int32_t s_w[kMetWaves];
  __shared__ unsigned long long s_u[kMetWaves], s_p[kMetWaves];
  const int t = threadIdx.x, tile = blockIdx.x;
  // the tiles before this one: their negatives, and NP at the last run start among them
  int32_t negbase = 0, best = -1;
  for (int j0 = 0; j0 < tile; j0 += kMetThreads) {
    const int j = j0 + t;
    const int32_t v = j < tile ? tile_neg[j] : 0;
    int32_t total;
    const int32_t ex = met_exscan(v, s_w, &total);
    if (j < tile) {
      const int32_t ls = tile_ls[j];
      if (ls >= 0) best = max(best, negbase + ex + ls);
    }
    negbase += total;
  }
  const int32_t carry = met_block_max(best, s_w);

  TileItems it;
  met_load_items(rec, count, (int64_t)tile * kMetTile + (int64_t)t * kMetIPT, it);
  int32_t total;
  const int32_t ex = met_exscan(it.cnt, s_w, &total);
  int32_t run = negbase + ex, last = -1;
#pragma unroll
  for (int i = 0; i < kMetIPT; ++i) {
    if (it.start[i]) last = run;
    run += it.neg[i] ? 1 : 0;
  }
  int32_t cur = max(carry, met_exmaxscan(last, s_w));  // NP at the start of the run in progress
  run = negbase + ex;
  unsigned long long u2 = 0ull, p = 0ull;
#pragma unroll
  for (int i = 0; i < kMetIPT; ++i) {
    if (it.start[i]) cur = run;
    if (it.neg[i]) {
      ++run;
    } else if (it.live[i]) {
      ++p;
      u2 += (unsigned long long)run + (unsigned long long)cur;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    u2 += __shfl_xor(u2, o, kWave);
    p += __shfl_xor(p, o, kWave);
  }
  if ((t & (kWave - 1)) == 0) {
    s_u[t / kWave] = u2;
    s_p[t / kWave] = p;
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long U = 0ull, P = 0ull;
    for (int j = 0; j < kMetWaves; ++j) {
      U += s_u[j];
      P += s_p[j];
    }
    // integer adds: the order is irrelevant
    if (U) atomicAdd(&state->u2, U);
    if (P) atomicAdd(&state->pos, P);
    if (total) atomicAdd(&state->neg, (unsigned long long)total);
  }
}

// ------------------------------------------------------------------ host side ---------
struct MetLayout {
  uint64_t* tmp;      // [cap] the sort's second buffer
  int32_t* hist;      // [tiles][512]
  int32_t* tile_neg;  // [tiles]
  int32_t* tile_ls;   // [tiles]
  double* partials;   // [ceil(cap / kAppChunk)][2]
  size_t total;
};

static size_t met_layout(int64_t cap, char* base, MetLayout* L) {
  const int64_t tiles = ceil_div(cap, kMetTile);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (size_t)align_up((int64_t)bytes, 256);
    return base ? base + o : nullptr;
  };
  L->tmp = reinterpret_cast<uint64_t*>(take(sizeof(uint64_t) * cap));
  L->hist = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)(1 << kMetFirstBits) * tiles));
  L->tile_neg = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * tiles));
  L->tile_ls = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * tiles));
  L->partials = reinterpret_cast<double*>(take(sizeof(double) * 2 * ceil_div(cap, kAppChunk)));
  L->total = off;
  return off;
}

static bool met_cap_ok(int64_t cap) { return cap >= 1 && cap <= INT32_MAX; }

static int met_check_ws(const char* who, int64_t cap, const void* ws, int64_t ws_bytes) {
  MetLayout L;
  const int64_t need = (int64_t)met_layout(cap, nullptr, &L);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) {
    set_error("%s: workspace %lld < %lld bytes (or null / not 16-B aligned)", who,
              (long long)ws_bytes, (long long)need);
    return CTR_ERR_WORKSPACE;
  }
  return CTR_OK;
}

template <typename LT>
static void met_launch_append(const AppendArgs& a, hipStream_t st) {
  if (a.n <= kAppSingleMax) {
    hipLaunchKernelGGL((metrics_append_kernel<LT, true>), 1, kAppThreads, 0, st, a);
  } else {
    const int nb = (int)ceil_div(a.n, kAppChunk);
    hipLaunchKernelGGL((metrics_append_kernel<LT, false>), (unsigned)nb, kAppThreads, 0, st, a);
    hipLaunchKernelGGL(metrics_combine_kernel, 1, kMetThreads, 0, st, a, nb);
  }
}

template <int BITS>
static void met_launch_pass(const MetSortPass& p, hipStream_t st) {
  hipLaunchKernelGGL(metrics_hist_kernel<BITS>, (unsigned)p.n_tiles, kMetThreads, 0, st, p);
  hipLaunchKernelGGL(metrics_scatter_kernel<BITS>, (unsigned)p.n_tiles, kMetThreads, 0, st, p);
}

}  // namespace ctr

using namespace ctr;

extern "C" int ctr_metrics_tile(void) { return kMetTile; }

extern "C" int64_t ctr_metrics_workspace_bytes(int64_t cap) {
  if (!met_cap_ok(cap)) return 0;
  MetLayout L;
  return (int64_t)met_layout(cap, nullptr, &L);
}

extern "C" int ctr_metrics_reset(void* state, ctr_stream_t stream) {
  CTR_REQUIRE(state, "ctr_metrics_reset: null state");
  CTR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0,
              "ctr_metrics_reset: state is not 8-byte aligned");
  CTR_HIP_CHECK(hipMemsetAsync(state, 0, CTR_METRICS_STATE_BYTES, as_stream(stream)));
  return CTR_OK;
}

extern "C" int ctr_metrics_append(int64_t cap, int64_t offset, int64_t n, const float* pred,
                                  int64_t stride, const void* labels, int label_type,
                                  const float* rewards, int with_loss, uint64_t* records,
                                  void* ws, int64_t ws_bytes, void* state, ctr_stream_t stream) {
  CTR_REQUIRE(met_cap_ok(cap), "ctr_metrics_append: cap=%lld outside [1, 2^31)", (long long)cap);
  CTR_REQUIRE(offset >= 0 && n >= 0 && offset <= cap && n <= cap - offset,
              "ctr_metrics_append: offset %lld + n %lld > cap %lld (or negative)",
              (long long)offset, (long long)n, (long long)cap);
  CTR_REQUIRE(label_type == CTR_LABEL_F32 || label_type == CTR_LABEL_I32 ||
                  label_type == CTR_LABEL_I64,
              "ctr_metrics_append: label type %d is not fp32 (0), int32 (1) or int64 (2)",
              label_type);
  CTR_REQUIRE(stride >= 1, "ctr_metrics_append: stride %lld < 1", (long long)stride);
  CTR_REQUIRE(records && state, "ctr_metrics_append: null records / state");
  CTR_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(state) & 7) == 0,
              "ctr_metrics_append: records / state not 8-byte aligned");
  int rc = met_check_ws("ctr_metrics_append", cap, ws, ws_bytes);
  if (rc != CTR_OK) return rc;
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(pred && labels, "ctr_metrics_append: null predictions / labels");
  MetLayout L;
  met_layout(cap, static_cast<char*>(ws), &L);
  AppendArgs a;
  a.pred = pred;
  a.stride = stride;
  a.labels = labels;
  a.rewards = rewards;
  a.n = n;
  a.rec = records + offset;
  a.with_loss = with_loss ? 1 : 0;
  a.partials = L.partials;
  a.state = static_cast<MetricsState*>(state);
  hipStream_t st = as_stream(stream);
  if (label_type == CTR_LABEL_F32) met_launch_append<float>(a, st);
  else if (label_type == CTR_LABEL_I32) met_launch_append<int32_t>(a, st);
  else met_launch_append<int64_t>(a, st);
  CTR_LAUNCH_CHECK("ctr_metrics_append");
  return CTR_OK;
}

extern "C" int ctr_metrics_auc(int64_t cap, int64_t count, uint64_t* records, void* ws,
                               int64_t ws_bytes, void* state, ctr_stream_t stream) {
  CTR_REQUIRE(met_cap_ok(cap), "ctr_metrics_auc: cap=%lld outside [1, 2^31)", (long long)cap);
  CTR_REQUIRE(count >= 0 && count <= cap, "ctr_metrics_auc: count %lld outside [0, cap=%lld]",
              (long long)count, (long long)cap);
  CTR_REQUIRE(records && state, "ctr_metrics_auc: null records / state");
  CTR_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(state) & 7) == 0,
              "ctr_metrics_auc: records / state not 8-byte aligned");
  int rc = met_check_ws("ctr_metrics_auc", cap, ws, ws_bytes);
  if (rc != CTR_OK) return rc;
  if (count == 0) return CTR_OK;
  MetLayout L;
  met_layout(cap, static_cast<char*>(ws), &L);
  hipStream_t st = as_stream(stream);
  MetricsState* s = static_cast<MetricsState*>(state);
  CTR_HIP_CHECK(hipMemsetAsync(s, 0, 3 * sizeof(unsigned long long), st));  // u2, pos, neg
  MetSortPass p;
  p.hist = L.hist;
  p.count = count;
  p.n_tiles = (int)ceil_div(count, kMetTile);
  uint64_t* buf[2] = {records, L.tmp};
  int shift = 0;
  for (int pass = 0; pass < kMetPasses; ++pass) {  // an even number: ends in records
    p.in = buf[pass & 1];
    p.out = buf[(pass & 1) ^ 1];
    p.shift = shift;
    if (pass == 0) {
      met_launch_pass<kMetFirstBits>(p, st);
      shift += kMetFirstBits;
    } else {
      met_launch_pass<kMetBits>(p, st);
      shift += kMetBits;
    }
    CTR_LAUNCH_CHECK("ctr_metrics_auc (sort)");
  }
  hipLaunchKernelGGL(metrics_tile_count_kernel, (unsigned)p.n_tiles, kMetThreads, 0, st, records,
                     count, L.tile_neg, L.tile_ls);
  hipLaunchKernelGGL(metrics_reduce_kernel, (unsigned)p.n_tiles, kMetThreads, 0, st, records,
                     count, L.tile_neg, L.tile_ls, s);
  CTR_LAUNCH_CHECK("ctr_metrics_auc (reduce)");
  return CTR_OK;
}
