/*
 * ctr_hip.h — C ABI of libctr_hip.so, the MI355X (gfx950) hot path of
 * jqsl2012/RL_CTR_Prediction's CTR training step.
 *
 * Scope: the multi-field sparse->embedding gather, the FM
 * interaction (sum-square trick) and linear term, the DeepFM MLP head, the log-loss
 * (BCE after sigmoid) backward, the embedding scatter-add, the coupled-L2 Adam step,
 * Feature_Embedding's pairwise inner products and the REINFORCE loss of PG_model.
 *
 * Conventions (every entry point):
 *   - plain device pointers and sizes, row-major, fp32 unless stated; index arrays are
 *     int32 (CTR_IDX_I32) or int64 (CTR_IDX_I64, what the reference's LongTensor holds);
 *   - all work is enqueued on `stream` (a hipStream_t; NULL = legacy default stream);
 *     nothing synchronises, nothing allocates; scratch is caller-owned and sized by the
 *     matching *_workspace_bytes() query;
 *   - return CTR_OK (0) or a CTR_ERR_* code; ctr_last_error() then holds a thread-local
 *     message. Out-of-range feature ids never fault: the kernel reads row 0 instead and
 *     ORs CTR_EFLAG_INDEX into *err_flag (optional device int32), the analogue of
 *     nn.Embedding's "index out of range" error, checked by the host when it chooses.
 */
#ifndef CTR_HIP_H
#define CTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ctr_stream_t; /* hipStream_t */

enum ctr_status {
  CTR_OK = 0,
  CTR_ERR_INVALID = 1,     /* argument out of contract */
  CTR_ERR_HIP = 2,         /* HIP runtime / launch error */
  CTR_ERR_WORKSPACE = 3,   /* scratch smaller than the *_workspace_bytes() answer */
  CTR_ERR_UNSUPPORTED = 4  /* shape this build does not handle */
};

enum ctr_idx_type { CTR_IDX_I32 = 0, CTR_IDX_I64 = 1 };

enum ctr_err_flag {
  CTR_EFLAG_INDEX = 1,    /* a feature id outside [0, V) */
  CTR_EFLAG_CAPACITY = 2  /* a row-sharded exchange run longer than its capacity */
};

/* GEMM epilogues (ctr_gemm_f32). */
enum ctr_epilogue {
  CTR_EPI_NONE = 0,            /* C = A.B                                                  */
  CTR_EPI_BIAS = 1,            /* C = A.B + bias[n]                                        */
  CTR_EPI_BIAS_RELU = 2,       /* C = relu(A.B + bias[n])                                  */
  CTR_EPI_BIAS_RELU_DROP = 3,  /* C = dropout(relu(A.B + bias[n]); p, seed, offset)        */
  CTR_EPI_GRAD_MASK = 4        /* C = aux[m,n] > 0 ? (A.B) * scale : 0  (relu+dropout bwd) */
};

int ctr_abi_version(void);
const char* ctr_last_error(void);
/* Number of visible HIP devices (0 on a host without a GPU); never initialises a context
 * beyond hipGetDeviceCount. */
int ctr_device_count(void);
/* A stream whose kernels run only on the CUs set in mask[0 .. n_words) (bit c % 32 of word
 * c / 32 = CU c in the driver's numbering; hipExtStreamCreateWithCUMask), and its release.
 * The mask holds for launches on that stream, eager or as the root of a graph launched on
 * it, not for a graph branch forked onto it (tools/cumask_probe.hip). Measured and not
 * kept: the weight-gradient side stream on it (CTR_WGRAD_CU_FRAC); no product
 * code uses it any more. No reference counterpart. */
int ctr_stream_create_cu_masked(const uint32_t* mask, int n_words, ctr_stream_t* out);
int ctr_stream_destroy(ctr_stream_t stream);

/* ---------------------------------------------------------------- A3: gather ---------
 * out[i, :] = table[idx[i], :]  — nn.Embedding.forward. n = 0 is a no-op (idx and out may
 * be NULL: an empty tensor has no storage).
 * Replaces: p_model.py:47,303,320 and Feature_embedding.py:52 (self.feature_embedding(x)). */
int ctr_embedding_gather(const float* table, int64_t V, int K, const void* idx, int idx_type,
                         int64_t n, float* out, int32_t* err_flag, ctr_stream_t stream);

/* ------------------------------------------------------ A1/A2/A4: FM forward ---------
 * Fused gather + FM second order + linear term for B examples of F fields:
 *   z[b]      = bias[0] + sum_f lin[x_bf] + 0.5 * sum_k ((sum_f E[x_bf,k])^2 - sum_f E[x_bf,k]^2)
 *   sum_e     [B,K]   sum_f E[x_bf,:]      (optional; the backward needs it)
 *   emb_out   [B,F*K] E[x_bf,:] flattened  (optional; DeepFM's MLP input)
 * If labels != NULL the BCE-after-sigmoid head is fused (FM model):
 *   p[b] = sigmoid(z[b]); loss_elem[b] = BCE(p, y) (log clamped at -100);
 *   gz[b] = d(mean BCE)/dz with the reference's UNFUSED formula in ATen's operation order,
 *           mean_div = the batch the mean runs over (B, or B_global under data parallel):
 *           g_p = ((p-y)/max((1-p)p, 1e-12))/mean_div; gz = (g_p*(1-p))*p.
 *   p, loss_elem, gz may then be non-NULL individually.
 * Replaces: p_model.py:40-57 (FM.forward), 296-313 (DeepFM.to_fm), nn.BCELoss at
 * all_main/pretrain_main.py:74,139. */
int ctr_fm_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                   const float* emb, const float* lin, const float* bias,
                   float* z, float* sum_e, float* emb_out,
                   const float* labels, float mean_div,
                   float* p, float* loss_elem, float* gz,
                   int32_t* err_flag, ctr_stream_t stream);

/* LR forward: z[b] = bias[0] + sum_f lin[x_bf], the F weights added in field order
 * (((w_0 + w_1) + w_2) + ...), and p = sigmoid(z); with labels the BCE head of ctr_fm_forward
 * (p, loss_elem, gz). z, p, loss_elem and gz may be NULL individually. 1 <= F <= 64; a row is
 * a group of lanes (several rows per wave when F < 64), never one thread. Out-of-range ids, null
 * pointers and bad sizes as ctr_fm_forward.
 * Replaces: p_model.py:18-26 (LR.forward), nn.BCELoss at all_main/pretrain_main.py:74. */
int ctr_lr_forward(const void* idx, int idx_type, int64_t B, int F, int64_t V, const float* lin,
                   const float* bias, float* z, float* p, const float* labels, float mean_div,
                   float* loss_elem, float* gz, int32_t* err_flag, ctr_stream_t stream);

/* BCE after sigmoid on precomputed logits (same formulas as the fused FM head).
 * Replaces: torch.sigmoid (p_model.py:55,324) + nn.BCELoss (pretrain_main.py:74). */
int ctr_bce_sigmoid(const float* z, const float* labels, int64_t B, float mean_div,
                    float* p, float* loss_elem, float* gz, ctr_stream_t stream);

/* DeepFM output head: z[b] = z_fm[b] + h[b,:].w_out + b_out[0]; then the BCE head as above.
 * dh_pre[b,j] = h[b,j] > 0 ? gz[b]*w_out[j]*drop_scale : 0  (grad through the last
 * Linear, the Dropout and the ReLU that produced h; drop_scale = 1/(1-p) or 1 in eval).
 * Replaces: p_model.py:322-324 (mlp[6] Linear(200,1) + sum + sigmoid), pretrain_main.py:74. */
int ctr_deepfm_head(const float* h, int64_t B, int H, const float* w_out, const float* b_out,
                    const float* z_fm, const float* labels, float mean_div, float drop_scale,
                    float* z, float* p, float* loss_elem, float* gz, float* dh_pre,
                    ctr_stream_t stream);

/* -------------------------------------------------------- MLP: fp32 MFMA GEMM ---------
 * C[M,N] = op(A)[M,K] . op(B)[K,N] with epilogue `epi` (enum ctr_epilogue).
 * trans_a = 0: A stored [M,K] (lda >= K); 1: A stored [K,M] (lda >= M).
 * trans_b = 0: B stored [K,N] (ldb >= N); 1: B stored [N,K] (ldb >= K)  (nn.Linear weight).
 * K == 0 is allowed (A and B may then be NULL) and yields the epilogue of 0: zeros, bias[n],
 * relu(bias[n]), ... Leading dimensions may exceed the extents; elements between a row's
 * extent and its stride are never read (A, B, aux) nor written (C). The alignment of A, B
 * and C and lda/ldb/ldc % 4 select a staging / store path (16-byte LDS-DMA and float4 stores,
 * or register staging and scalar stores), never a result: the same operands give the same
 * bits at any base address and leading dimension.
 * Dropout keeps element (m,n) iff hash(seed, offset + m*N + n) >= p*2^32 and scales by
 * 1/(1-p), where offset += (*step_ptr) << 32 when step_ptr != NULL (a per-step mask read
 * on the device, for HIP-graph replay). The counter runs over the logical matrix (m*N + n,
 * not m*ldc + n) in uint64 arithmetic mod 2^64; hash = the high 32 bits of the
 * (counter+1)-th splitmix64 output for state `seed`; p*2^32 is formed in double from the
 * fp32 p, clamped to 2^32 - 1 and truncated. `scale` is used by CTR_EPI_GRAD_MASK (aux is
 * read at aux[m*ldaux + n], ldaux >= N). Split-K (long K, few tiles) uses `ws`.
 * Replaces: nn.Linear / ReLU / Dropout of DeepFM.mlp (p_model.py:276-293) and of
 * PG_model.Net.mlp (PG_model.py:41-51), forward and autograd backward (dX and dW). */
int64_t ctr_gemm_f32_workspace_bytes(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K);
/* ctr_gemm_f32 = ctr_gemm_f32_ex(CTR_GEMM_AUTO, ...). */
int ctr_gemm_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K,
                 const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc, int epi, const float* bias,
                 const float* aux, int64_t ldaux, float scale,
                 float drop_p, uint64_t seed, uint64_t offset, const int32_t* step_ptr,
                 void* ws, int64_t ws_bytes, ctr_stream_t stream);

/* GEMM algorithms (same contract, same fp32 operands and outputs):
 *  CTR_GEMM_EXACT_F32  v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation.
 *  CTR_GEMM_SPLIT_BF16 each fp32 operand split exactly into three bf16 planes
 *                      (x = x0 + x1 + x2, RNE); the six partial products with
 *                      i + j <= 2 on v_mfma_f32_32x32x16_bf16, fp32 accumulation. The
 *                      dropped terms are <= 2^-23 |a*b| per product (one fp32 multiply's
 *                      rounding); 2.7x the fp32 matrix rate.
 *  CTR_GEMM_AUTO       SPLIT_BF16 unless the environment sets CTR_GEMM_ALGO=exact. */
enum ctr_gemm_algo { CTR_GEMM_AUTO = 0, CTR_GEMM_EXACT_F32 = 1, CTR_GEMM_SPLIT_BF16 = 2 };
int64_t ctr_gemm_f32_ex_workspace_bytes(int algo, int trans_a, int trans_b, int64_t M, int64_t N,
                                        int64_t K);
int ctr_gemm_f32_ex(int algo, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K,
                    const float* A, int64_t lda, const float* B, int64_t ldb,
                    float* C, int64_t ldc, int epi, const float* bias,
                    const float* aux, int64_t ldaux, float scale,
                    float drop_p, uint64_t seed, uint64_t offset, const int32_t* step_ptr,
                    void* ws, int64_t ws_bytes, ctr_stream_t stream);
/* The algorithm CTR_GEMM_AUTO (or any value) resolves to in this process. */
int ctr_gemm_resolved_algo(int algo);

/* ------------------------------------------- A2: MLP GEMM on pre-split planes -------
 * The fused trainer's MLP GEMMs (the six products of DeepFM's / InnerPNN's MLP per step,
 * p_model.py:276-293,322 forward and backward). An fp32 matrix travels as its exact
 * three-plane bf16 split x = x0 + x1 + x2 (CTR_GEMM_SPLIT_BF16's numerics), written once
 * by its producer, so the GEMM stages operands by LDS-DMA without any split work.
 *
 * ctr_planes: bf16 bits [3][rows][cols] with row stride `ld` and plane stride
 * `plane_stride` (elements); `rows`/`cols` = the allocated storage extents. CONTRACT: the
 * storage beyond the matrix's logical extent is ZERO and stays zero (the GEMM reads whole
 * 32-deep k tiles), ld % 8 == 0, data 16-B aligned.
 *
 * ctr_split_planes: planes of src [rows, cols] (row stride ld); writes the valid region.
 *
 * ctr_gemm_planes: C[M,N] = A.B with the ctr_gemm_f32 epilogues. Orientation per operand:
 *   a_rc = 0: A stored [M][K] (k contiguous)     a_rc = 1: A stored [K][M] (A^T product)
 *   b_rc = 0: B stored [N][K] (nn.Linear weight) b_rc = 1: B stored [K][N]
 * Storage must cover align_up(K, 32) along k, zero-padded (K == 0: one all-zero k tile, the
 * result is the epilogue of 0). ldc >= N and, for CTR_EPI_GRAD_MASK, ldaux >= N; C's
 * alignment and ldc % 4 select a store path, never a result; the dropout counter is m*N + n
 * as in ctr_gemm_f32. Outputs: C (fp32, ldc) and/or Cp
 * (the planes of the epilogue's result, for the next GEMM). Split-K scratch is sized by
 * ctr_gemm_planes_workspace_bytes. ctr_gemm_planes_config reports the tiling chosen
 * (tuning and tests). */
typedef struct ctr_planes {
  void* data;
  int64_t ld;
  int64_t plane_stride;
  int64_t rows;
  int64_t cols;
} ctr_planes;
int ctr_split_planes(const float* src, int64_t rows, int64_t cols, int64_t ld,
                     const ctr_planes* dst, ctr_stream_t stream);
int64_t ctr_gemm_planes_workspace_bytes(int a_rc, int b_rc, int64_t M, int64_t N, int64_t K);
int ctr_gemm_planes(int a_rc, int b_rc, int64_t M, int64_t N, int64_t K,
                    const ctr_planes* A, const ctr_planes* B, float* C, int64_t ldc,
                    const ctr_planes* Cp, int epi, const float* bias, const float* aux,
                    int64_t ldaux, float scale, float drop_p, uint64_t seed, uint64_t offset,
                    const int32_t* step_ptr, void* ws, int64_t ws_bytes, ctr_stream_t stream);
int ctr_gemm_planes_config(int a_rc, int b_rc, int64_t M, int64_t N, int64_t K, int* tile,
                           int* splits, int* bm, int* bn);
/* ctr_gemm_planes_lastcol: ctr_gemm_planes whose result column N-1 is written to
 * last_col[m] (m < M) instead of C, which then holds N-1 columns (ldc >= N-1). With a B
 * operand whose column N-1 is all ones (a ones column in the planes' zero padding), a weight
 * gradient dW = G^T X and its bias gradient db = colsum(G) come out of ONE GEMM.
 * Replaces: the mlp.0 / mlp.3 weight AND bias gradients of p_model.py:276-293 backward. */
int ctr_gemm_planes_lastcol(int a_rc, int b_rc, int64_t M, int64_t N, int64_t K,
                            const ctr_planes* A, const ctr_planes* B, float* C, int64_t ldc,
                            const ctr_planes* Cp, int epi, const float* bias, const float* aux,
                            int64_t ldaux, float scale, float drop_p, uint64_t seed,
                            uint64_t offset, const int32_t* step_ptr, float* last_col, void* ws,
                            int64_t ws_bytes, ctr_stream_t stream);

/* The producers of the MLP's GEMM operands writing planes directly (no fp32 round trip):
 * ctr_fm_forward_planes: ctr_fm_forward (no BCE head; DeepFM's FM part) whose flattened
 *   embeddings (emb_out [B, F*K]) are written as planes; needs K % 4 == 0, (K/4) | 64,
 *   F <= 64. Replaces: p_model.py:303,320 (the two gathers of DeepFM.forward).
 * ctr_deepfm_head_planes: ctr_deepfm_head with labels, writing dh_pre [B, H] in fp32 (dh_pre
 *   may be NULL: the planes only) and as planes (the dH1 / dW1 GEMM operand). Replaces:
 *   p_model.py:290-293,322 backward. */
int ctr_fm_forward_planes(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                          const float* emb, const float* lin, const float* bias, float* z,
                          float* sum_e, const ctr_planes* emb_planes, int32_t* err_flag,
                          ctr_stream_t stream);
int ctr_deepfm_head_planes(const float* h, int64_t B, int H, const float* w_out,
                           const float* b_out, const float* z_fm, const float* labels,
                           float mean_div, float drop_scale, float* z, float* p, float* loss_elem,
                           float* gz, float* dh_pre, const ctr_planes* dh_planes,
                           ctr_stream_t stream);

/* Deterministic reductions (fixed order; identical bits run to run).
 * ctr_sum_f32:    out[0] = scale * sum_i x[i]
 * ctr_colsum_f32: out[n] = scale * sum_m (row_w ? row_w[m] : 1) * X[m,n]   (bias / dW of
 *                 a 1-row Linear). */
int64_t ctr_reduce_workspace_bytes(int64_t M, int64_t N);
int ctr_sum_f32(const float* x, int64_t n, float scale, float* out, void* ws, int64_t ws_bytes,
                ctr_stream_t stream);
int ctr_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ldx, const float* row_w,
                   float scale, float* out, void* ws, int64_t ws_bytes, ctr_stream_t stream);
/* Up to 8 ctr_colsum_f32 jobs in one launch pair, each output bitwise ctr_colsum_f32's
 * (same row partition and order): the DeepFM step's bias gradients (colsum dH1, dH2), the
 * last layer's weight gradient (gz-weighted colsum of H2) and its bias (colsum of gz). */
typedef struct ctr_colsum_job {
  const float* X;
  int64_t M, N, ldx;
  const float* row_w;
  float scale;
  float* out;
} ctr_colsum_job;
int64_t ctr_colsum_multi_workspace_bytes(int n_jobs, const ctr_colsum_job* jobs);
int ctr_colsum_multi_f32(int n_jobs, const ctr_colsum_job* jobs, void* ws, int64_t ws_bytes,
                         ctr_stream_t stream);

/* dst[c * ld_dst + r] = src[r * ld_src + c] (r < rows, c < cols), bit-exact copy: dH1^T and
 * X^T for the k-contiguous dW0 = dH1^T X GEMM of DeepFM / IPNN (p_model.py:279-293, the
 * weight gradient autograd forms for mlp.0). */
int ctr_transpose_f32(const float* src, int64_t rows, int64_t cols, int64_t ld_src, float* dst,
                      int64_t ld_dst, ctr_stream_t stream);

/* ------------------------------------------------ A3: embedding scatter-add -----------
 * A sparse plan groups the S = B*F slots (slot s = b*F + f) of a batch by feature id.
 * All arrays are caller-owned device buffers of S int32 (seg_offsets: S+1, num_unique: 1):
 *   sorted_slots  slot ids ordered by (row, slot) — a STABLE sort, so each row's slots keep
 *                 the order embedding_dense_backward accumulates them in;
 *   sorted_rows   the row of each sorted position;
 *   pos_seg       the segment (unique-row ordinal) of each sorted position;
 *   unique_rows   the distinct rows ascending, first *num_unique valid;
 *   seg_offsets   row u owns sorted positions [seg_offsets[u], seg_offsets[u+1]).
 * Index work: bit-exact (tests compare with numpy.unique). Replaces the grouping inside
 * embedding_dense_backward (autograd through p_model.py:47,54,303,311,320). */
typedef struct ctr_sparse_plan {
  int64_t S;
  int32_t* sorted_slots;
  int32_t* sorted_rows;
  int32_t* pos_seg;
  int32_t* unique_rows;
  int32_t* seg_offsets;
  int32_t* num_unique;
} ctr_sparse_plan;

int64_t ctr_sparse_plan_workspace_bytes(int64_t S, int64_t V);
/* Row sharding: rank j owns ids [j*shard_rows, (j+1)*shard_rows).
 * ctr_plan_slot_to_unique: slot_to_unique[s] = the unique-row ordinal of slot s (int32[S]);
 *   a forward over the rows received from their owners (compacted in unique order) reads
 *   them with these ids.
 * ctr_plan_shard_counts: counts[j] (int64[n_shards]) = how many of the plan's unique rows
 *   shard j owns; the unique rows are ascending, so they leave grouped by owner. */
int ctr_plan_slot_to_unique(const ctr_sparse_plan* plan, int32_t* slot_to_unique,
                            ctr_stream_t stream);
int ctr_plan_shard_counts(const ctr_sparse_plan* plan, int64_t shard_rows, int n_shards,
                          int64_t* counts, ctr_stream_t stream);
/* ctr_plan_shard_counts_max: the same counts and, in max_out[0] (int64, may be NULL), their
 * maximum — the step's largest per-owner run, which sizes the row-sharded exchange (one
 * launch; max_out needs n_shards <= 15). */
int ctr_plan_shard_counts_max(const ctr_sparse_plan* plan, int64_t shard_rows, int n_shards,
                              int64_t* counts, int64_t* max_out, ctr_stream_t stream);
/* ctr_sparse_plan_build_runs: the plan (bit-identical to ctr_sparse_plan_build's) of the ids an
 * owner shard receives in a row-sharded step: n_runs <= 8 runs of run_len int32 ids
 * (ids[j*run_len + i]), each run ascending with every row at most once, padded at its end with
 * the spare row n_rows - 1 (repeated); rows in [0, n_rows). mask: uint32[ceil(n_rows/4)], zero
 * on entry and left zero (a per-row bitmask of the requesting runs); ws: caller scratch of
 * ctr_sparse_plan_runs_workspace_bytes bytes. plan->S must be n_runs * run_len. */
int64_t ctr_sparse_plan_runs_workspace_bytes(int n_runs, int64_t run_len, int64_t n_rows);
int ctr_sparse_plan_build_runs(const int32_t* ids, int n_runs, int64_t run_len, int64_t n_rows,
                               const ctr_sparse_plan* plan, uint32_t* mask, void* ws,
                               int64_t ws_bytes, ctr_stream_t stream);
/* ids[i] += delta (global row ids <-> shard-local row ids). */
int ctr_ids_add(int32_t* ids, int64_t n, int32_t delta, ctr_stream_t stream);
/* Fixed-capacity exchange of a row-sharded step (no reference counterpart: the reference
 * runs on one device, all_main/pretrain_main.py:232; this is the exchange SURVEY.md §8e
 * adds around nn.Embedding's gather / embedding_dense_backward, p_model.py:47,303,311,320).
 * Every (requester, owner j) pair moves `capacity` rows, so the all-to-alls are equal-split
 * and their sizes depend on the capacity alone (a step is capturable in a HIP graph).
 * ctr_shard_pack_ids: send[j*capacity + i] (int32) = the i-th unique row of the plan owned by
 *   shard j as an owner-local id, or past that run the owner's spare row (its row count,
 *   min(shard_rows, V - j*shard_rows)); counts[j] / offsets[j] (int32[n_shards]) = the run's
 *   length and start in the plan's unique rows; a run longer than capacity ORs
 *   CTR_EFLAG_CAPACITY into *err_flag.
 * ctr_shard_runs_copy: rows of `width` floats between the compact order (run j at offsets[j])
 *   and the padded layout (run j at j*capacity): pack = 1 writes every padded row (zeros past
 *   a run), pack = 0 writes the runs back to their compact places. */
/* ctr_batch_stage_copy: one launch copying a batch into its fixed input slot — n0 bytes src0 ->
 * dst0 (the ids) and n1 bytes src1 -> dst1 (the labels; n1 = 0: none); device pointers, bitwise
 * copies. The staging of the reference's per-iteration batch (all_main/pretrain_main.py:71-74,
 * `for x, y in loader: x.to(device)`) ahead of the step that trains on it. */
int ctr_batch_stage_copy(void* dst0, const void* src0, int64_t n0, void* dst1, const void* src1,
                         int64_t n1, ctr_stream_t stream);
int ctr_shard_pack_ids(const ctr_sparse_plan* plan, int64_t shard_rows, int64_t V, int n_shards,
                       int64_t capacity, int32_t* send, int32_t* counts, int32_t* offsets,
                       int32_t* err_flag, ctr_stream_t stream);
int ctr_shard_runs_copy(const float* src, float* dst, int64_t width, int64_t capacity,
                        int n_shards, const int32_t* counts, const int32_t* offsets, int pack,
                        ctr_stream_t stream);
/* Cyclic row sharding (ABI v12): global row r belongs to shard r % n_shards as its local row
 * r / n_shards, so every shard owns rows of every feature field (the field-ordered vocabulary
 * of the reference's encoders, creat_data.py / data_.py, puts the high-cardinality fields in
 * the last row blocks: contiguous blocks leave one owner most of every batch's rows).
 * ctr_shard_permute_ids: in place, ids[i] = (r % n_shards) * shard_rows + r / n_shards — the
 *   space in which each shard's rows are one contiguous block [j*shard_rows, j*shard_rows+n_j),
 *   n_j = ceil((V - j) / n_shards); ids outside [0, V) raise CTR_EFLAG_INDEX and map to
 *   row 0. int64 or int32 ids (ids_is_64); the plan and the exchange then run on these ids.
 * ctr_shard_pack_ids_layout: ctr_shard_pack_ids over permuted ids; cyclic != 0: each owner's
 *   spare row is its cyclic row count n_j (blocks: as ctr_shard_pack_ids). */
int ctr_shard_permute_ids(void* ids, int ids_is_64, int64_t count, int64_t V, int n_shards,
                          int64_t shard_rows, int32_t* err_flag, ctr_stream_t stream);
int ctr_shard_pack_ids_layout(const ctr_sparse_plan* plan, int64_t shard_rows, int64_t V,
                              int n_shards, int cyclic, int64_t capacity, int32_t* send,
                              int32_t* counts, int32_t* offsets, int32_t* err_flag,
                              ctr_stream_t stream);
/* The same exchange with each row's linear weight in the same message: the padded buffer is
 * n_shards chunks of `chunk` floats (chunk >= capacity*K + capacity, a multiple of 4), chunk j
 * = [capacity rows of K floats][capacity linear weights][padding]; lin == NULL: rows only.
 * One equal-split all-to-all then moves rows and weights (and their gradients) together.
 * ctr_shard_gather_rows (owner): chunk j row i = (emb[ids[j*capacity+i]], lin[...]).
 * ctr_shard_rows_pack: chunk j row i = (rows[offsets[j]+i], lin[...]) for i < counts[j],
 *   zeros past it.  ctr_shard_rows_unpack: the reverse, for i < counts[j].
 * K % 4 == 0, 16-B aligned buffers. */
int ctr_shard_gather_rows(const float* emb, const float* lin, int K, const int32_t* ids,
                          int n_shards, int64_t capacity, int64_t chunk, float* out,
                          ctr_stream_t stream);
int ctr_shard_rows_pack(const float* rows, const float* lin, int K, int64_t capacity,
                        int64_t chunk, int n_shards, const int32_t* counts,
                        const int32_t* offsets, float* out, ctr_stream_t stream);
int ctr_shard_rows_unpack(const float* in, int K, int64_t capacity, int64_t chunk, int n_shards,
                          const int32_t* counts, const int32_t* offsets, float* rows, float* lin,
                          ctr_stream_t stream);
/* ctr_shard_row_grads: a row-sharded requester's per-row gradient sums (ctr_fm_embedding_grad
 * when gz != NULL, else ctr_segment_sum_rows over vals without linear sums) written straight
 * into the exchange chunks of ctr_shard_rows_pack's layout: unique row u of run j (the last
 * run with run_offsets[j] <= u) goes to row u - run_offsets[j] of chunk j, its linear sum
 * after the chunk's run_len rows (lin != 0). Rows past a run's count are not written (the
 * owner's spare row takes them). K % 4 == 0, 16-B aligned buffers. */
int ctr_shard_row_grads(const ctr_sparse_plan* plan, int F, int K, const float* emb,
                        const float* gz, const float* sum_e, const float* dx, const float* vals,
                        int lin, int n_runs, const int32_t* run_offsets, int64_t run_len,
                        int64_t chunk, float* out_chunks, void* ws, int64_t ws_bytes,
                        ctr_stream_t stream);
int ctr_sparse_plan_build(const void* idx, int idx_type, int64_t V, const ctr_sparse_plan* plan,
                          void* ws, int64_t ws_bytes, int32_t* err_flag, ctr_stream_t stream);
/* The same plan (bit-identical) for ids laid out as a [S/F][F] matrix (slot s = b*F + f: the
 * batch's feature fields as columns): each column sorted inside one workgroup, then merged —
 * 2 launches of work where a column's ids occupy a range of their own (the CTR layouts), and
 * exact for any ids. Falls back to ctr_sparse_plan_build for S/F > 8192 or F > 256. */
int ctr_sparse_plan_build_cols(const void* idx, int idx_type, int64_t V, int64_t F,
                               const ctr_sparse_plan* plan, void* ws, int64_t ws_bytes,
                               int32_t* err_flag, ctr_stream_t stream);

/* Segmented row sums over a plan, deterministic: each row's slots are summed in slot
 * order in chunks of 16 positions, chunk partials are then added in chunk order (hot
 * rows spread over many waves; identical bits run to run and rank to rank).
 *   ctr_fm_embedding_grad (FM / DeepFM backward, slot s = b*F + f):
 *     grad_rows[u,:] = sum_{s in row u} ((gz[b]*sum_e[b,:] - gz[b]*E[row,:]) + dx[s,:])
 *     grad_lin[u]    = sum_{s in row u} gz[b]
 *     dx (the MLP input gradient, [B, F*K]) is NULL for FM.
 *   ctr_segment_sum_rows (generic; multi-GPU exchange): out[u,:] = sum vals[s,:],
 *     out_lin[u] = sum vals_lin[s] (both optional-lin).
 * If rowmap != NULL also rowmap[row_u] = u (ctr_adam_embedding consumes and resets it).
 * Replaces: FM/DeepFM backward through p_model.py:47-54 / 303-311 / 320-322 and
 * embedding_dense_backward. */
int64_t ctr_segment_workspace_bytes(int64_t S, int K);
int ctr_fm_embedding_grad(const ctr_sparse_plan* plan, int F, int K, const float* emb,
                          const float* gz, const float* sum_e, const float* dx,
                          float* grad_rows, float* grad_lin, int32_t* rowmap, void* ws,
                          int64_t ws_bytes, ctr_stream_t stream);
int ctr_segment_sum_rows(const ctr_sparse_plan* plan, int K, const float* vals,
                         const float* vals_lin, float* out, float* out_lin, int32_t* rowmap,
                         void* ws, int64_t ws_bytes, ctr_stream_t stream);

/* Dense gradient for the autograd (drop-in) path: dense[V,K] (and dense_lin[V], optional)
 * must be zero on entry; dense[row_u,:] = grad_rows[u,:]. */
int ctr_rows_to_dense(const ctr_sparse_plan* plan, int K, const float* grad_rows,
                      const float* grad_lin, float* dense, float* dense_lin,
                      ctr_stream_t stream);

/* ---------------------------------------------------------------- A5: Adam -----------
 * torch.optim.Adam(lr, betas, eps, weight_decay) with coupled L2, one step, for EVERY
 * element (dense semantics). Host-computed step scalars (as torch computes them):
 *   step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t).
 * Per element: g += wd*p; m += (1-beta1)*(g-m); v = v*beta2 + (1-beta2)*g*g;
 *              p += -step_size * (m / (sqrt(v)/bc2_sqrt + eps))
 * (m, v bit-identical to torch's CPU Adam; the p step uses ~1-ulp hardware sqrt/rcp).
 * ctr_adam_dense:     g is a dense gradient (MLP, bias).
 * ctr_adam_embedding: the embedding table E[V,K] and the linear table w[V] in one pass;
 *   the gradient of row r is grad_rows[rowmap[r]] when rowmap[r] >= 0, else 0; rowmap
 *   entries read >= 0 are reset to -1. lin/m_lin/v_lin may be NULL (Feature tables w/o
 *   a linear term).
 * Device step (HIP-graph replay): with step_ptr != NULL the step t = *step_ptr is read on
 * the device and the scalars come from step_table (layout of ctr_adam_deferred_rows
 * below); step_size / bc2_sqrt are then ignored.
 * Replaces: torch.optim.Adam.step at all_main/pretrain_main.py:78,153. */
int ctr_adam_dense(float* p, const float* g, float* m, float* v, int64_t n, double step_size,
                   double bc2_sqrt, const float* step_table, const int32_t* step_ptr,
                   double beta1, double beta2, double eps, double weight_decay,
                   ctr_stream_t stream);
/* ctr_adam_dense_planes: ctr_adam_dense that also rewrites the bf16 planes (ctr_planes) of
 *   up to three row-major [rows, cols] sub-matrices of p (the MLP weights: p[offset + r*cols
 *   + c]) with the updated values, so the next step's plane GEMMs need no ctr_split_planes.
 *   offset % 4 == 0, n % 4 == 0, 16-B aligned vectors; any cols (a multiple of 4 is faster).
 *   Replaces: the same optimizer.step; the planes are this framework's GEMM operand format. */
typedef struct ctr_plane_view {
  int64_t offset;
  int64_t rows;
  int64_t cols;
  ctr_planes planes;
} ctr_plane_view;
int ctr_adam_dense_planes(float* p, const float* g, float* m, float* v, int64_t n,
                          double step_size, double bc2_sqrt, const float* step_table,
                          const int32_t* step_ptr, double beta1, double beta2, double eps,
                          double weight_decay, const ctr_plane_view* views, int n_views,
                          ctr_stream_t stream);
int ctr_adam_embedding(float* emb, float* m_emb, float* v_emb, float* lin, float* m_lin,
                       float* v_lin, int64_t V, int K, int32_t* rowmap,
                       const float* grad_rows, const float* grad_lin, double step_size,
                       double bc2_sqrt, const float* step_table, const int32_t* step_ptr,
                       double beta1, double beta2, double eps, double weight_decay,
                       ctr_stream_t stream);

/* Deferred-exact dense Adam (temporal blocking) — same results as ctr_adam_embedding,
 * bitwise. A row absent from a batch is updated with g = wd*p, a function of its own state;
 * last[r] (int32 [V], 0 at optimizer creation) records the step row r is current to, and
 * missed steps are replayed in registers with the same per-element arithmetic and the same
 * per-step scalars step_table[2t] = -lr/(1-beta1^t), step_table[2t+1] = 1/sqrt(1-beta2^t)
 * (fp32, host-computed in double as torch does; entries 0..step valid):
 *   ctr_adam_deferred_rows, grad_rows == NULL: bring the plan's unique rows to `step`
 *     (call before a forward pass reads them; catch-up to the last completed step);
 *   ctr_adam_deferred_rows, grad_rows != NULL: bring them to step-1 and apply step `step`
 *     with their gradient (grad_rows[u], grad_lin[u] for unique row u);
 *   ctr_adam_deferred_flush: bring every row to `step` (before anything else reads the
 *     tables: epoch end, checkpoint, evaluation).
 * ctr_adam_deferred_rows reads the step from *step_ptr on the device when step_ptr != NULL.
 * Replaces: torch.optim.Adam.step at all_main/pretrain_main.py:78 over nn.Embedding weights. */
int ctr_adam_deferred_rows(float* emb, float* m_emb, float* v_emb, float* lin, float* m_lin,
                           float* v_lin, int64_t V, int K, int32_t* last,
                           const ctr_sparse_plan* plan, const float* grad_rows,
                           const float* grad_lin, int64_t step, const int32_t* step_ptr,
                           const float* step_table, double beta1, double beta2, double eps,
                           double weight_decay, ctr_stream_t stream);
/* ctr_adam_deferred_entries: the owner side of a row-sharded step — for each unique row u of
 * `plan` (built over the received entries), g_u = the sum of vals[e] (and vals_lin[e]) over
 * its entries e in plan order (source rank, then position: sequential fp32 adds), then the
 * row replayed to step-1 and stepped with g_u (ctr_adam_deferred_rows with grad_rows = the
 * sums, in one launch). skip_row (e.g. the shard's spare row, the padding target) is left
 * untouched (-1: none). out [U][K] / out_lin [U] (optional): the sums. K % 4 == 0, (K/4) | 64.
 * run_len = 0: vals [entries][K], vals_lin [entries]; run_len > 0: vals is the chunked
 * exchange layout of ctr_shard_rows_pack (entry e = row e % run_len of chunk e / run_len,
 * chunk floats per chunk, the linear values after the rows; vals_lin unused). */
int ctr_adam_deferred_entries(float* emb, float* m_emb, float* v_emb, float* lin, float* m_lin,
                              float* v_lin, int64_t V, int K, int32_t* last,
                              const ctr_sparse_plan* plan, const float* vals,
                              const float* vals_lin, int64_t run_len, int64_t chunk,
                              int64_t skip_row, int64_t step,
                              const int32_t* step_ptr, const float* step_table, double beta1,
                              double beta2, double eps, double weight_decay, float* out,
                              float* out_lin, ctr_stream_t stream);
int ctr_adam_deferred_flush(float* emb, float* m_emb, float* v_emb, float* lin, float* m_lin,
                            float* v_lin, int64_t V, int K, int32_t* last, int64_t step,
                            const float* step_table, double beta1, double beta2, double eps,
                            double weight_decay, ctr_stream_t stream);
/* The catch-up of ctr_adam_deferred_rows (grad_rows == NULL) taken straight from a batch's
 * S feature ids, no sparse plan needed (the plan can then be built concurrently on another
 * stream): duplicates are resolved through `owner`, a caller-owned int32[V] scratch (no
 * initialisation needed); the target step is read from device memory (*step_ptr), so the
 * call can be captured in a HIP graph. Needs K % 4 == 0 and (K/4) | 64. */
int ctr_adam_deferred_catchup_ids(float* emb, float* m_emb, float* v_emb, float* lin,
                                  float* m_lin, float* v_lin, int64_t V, int K, int32_t* last,
                                  const void* idx, int idx_type, int64_t S, int32_t* owner,
                                  const int32_t* step_ptr, const float* step_table, double beta1,
                                  double beta2, double eps, double weight_decay,
                                  ctr_stream_t stream);
/* Fused scatter + deferred Adam (ws == 1, deferred mode): the segmented row sums of
 * ctr_fm_embedding_grad / ctr_segment_sum_rows with ctr_adam_deferred_rows(the sums,
 * step = *step_ptr) folded into the pass that finishes the rows spanning several chunks —
 * bitwise the same tables, one launch fewer, and the spanning rows' sums never round-trip
 * through memory. grad_rows / grad_lin (out / out_lin) are required scratch; with
 * keep_sums != 0 they hold every row's sum afterwards (else only the rows inside one
 * chunk). Needs K % 4 == 0, K <= 256.
 * Replaces: embedding_dense_backward + optimizer.step of all_main/pretrain_main.py:77-78. */
typedef struct ctr_deferred_table {
  float* emb;
  float* m_emb;
  float* v_emb;
  float* lin;    /* the linear table w[V] and its moments, or all NULL */
  float* m_lin;
  float* v_lin;
  int32_t* last; /* step each row is current to */
} ctr_deferred_table;
int ctr_fm_embedding_grad_adam(const ctr_sparse_plan* plan, int F, int K, const float* gz,
                               const float* sum_e, const float* dx,
                               const ctr_deferred_table* table, const int32_t* step_ptr,
                               const float* step_table, double beta1, double beta2, double eps,
                               double weight_decay, float* grad_rows, float* grad_lin,
                               int keep_sums, void* ws, int64_t ws_bytes, ctr_stream_t stream);
int ctr_segment_sum_rows_adam(const ctr_sparse_plan* plan, int K, const float* vals,
                              const float* vals_lin, const ctr_deferred_table* table,
                              const int32_t* step_ptr, const float* step_table, double beta1,
                              double beta2, double eps, double weight_decay, float* out,
                              float* out_lin, int keep_sums, void* ws, int64_t ws_bytes,
                              ctr_stream_t stream);

/* ------------------------------------------------ W&D (WideAndDeep) -------------------
 * p_model.WideAndDeep.forward (p_model.py:135-144): DeepFM without the second-order term,
 *   p = sigmoid((bias + sum_f lin[x_f]) + mlp(flat(embedding[x]))).
 * ctr_wd_forward: one launch writes the MLP input flat(E[x_b]) (F*K, bit-exact copies) as
 *   fp32 flat [B, >= F*K] (row stride ldf) and / or as its three bf16 planes (x_planes, valid
 *   region only: padding and a ones column stay as they are) — at least one of the two — and
 *   z_lin[b] = bias[0] + (lin[x_b0] + lin[x_b1] + ... in field order). No field sum, nothing
 *   else of size B*K. Any F >= 1, K >= 1 (16-byte accesses when K % 4 == 0 and the pointers
 *   and strides are 16-byte aligned, scalar ones otherwise: the same result either way); a
 *   row's outputs depend on that row alone. Ids outside [0, V) read row 0 and raise
 *   CTR_EFLAG_INDEX. B == 0: no launch.
 * ctr_wd_embedding_grad (slot s = b*F + f, the segmented sums above with their tree):
 *     grad_rows[u,:] = sum_{s in row u} dx[s,:]      (dx: the MLP input gradient [B, F*K])
 *     grad_lin[u]    = sum_{s in row u} gz[b]
 *   — ctr_segment_sum_rows over vals = dx, vals_lin = gz repeated F times, bit for bit;
 *   reads neither sum_e nor the table. rowmap as ctr_fm_embedding_grad's.
 * ctr_wd_embedding_grad_adam: the same sums with the deferred Adam apply fused in, as
 *   ctr_fm_embedding_grad_adam (K % 4 == 0, K <= 256, 16-byte aligned buffers; the linear
 *   table is required). ws: ctr_segment_workspace_bytes(S, K). */
int ctr_wd_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                   const float* emb, const float* lin, const float* bias, float* flat,
                   int64_t ldf, const ctr_planes* x_planes, float* z_lin, int32_t* err_flag,
                   ctr_stream_t stream);
int ctr_wd_embedding_grad(const ctr_sparse_plan* plan, int F, int K, const float* gz,
                          const float* dx, float* grad_rows, float* grad_lin, int32_t* rowmap,
                          void* ws, int64_t ws_bytes, ctr_stream_t stream);
int ctr_wd_embedding_grad_adam(const ctr_sparse_plan* plan, int F, int K, const float* gz,
                               const float* dx, const ctr_deferred_table* table,
                               const int32_t* step_ptr, const float* step_table, double beta1,
                               double beta2, double eps, double weight_decay, float* grad_rows,
                               float* grad_lin, int keep_sums, void* ws, int64_t ws_bytes,
                               ctr_stream_t stream);

/* Device step counters (int32[2]): ctr[0] = completed steps, ctr[1] = the step in flight.
 * ctr_step_begin: ctr[1] = ctr[0] + 1;  ctr_step_end: ctr[0] = ctr[1], ctr[1] += 1. A
 * counter initialised to {0, 1} therefore needs no ctr_step_begin (one launch less per
 * step); within a step both values are constant, so kernels on several streams can read
 * them: the catch-up and the dropout stream read ctr[0], the Adam apply ctr[1]. */
int ctr_step_begin(int32_t* step_ctr, ctr_stream_t stream);
int ctr_step_end(int32_t* step_ctr, ctr_stream_t stream);
/* ctr_step_end_loss: ctr_step_end, and loss_sum[0] += (double)loss[0] — the driver's epoch
 *   loss accumulated on the device (fp64, in step order: bitwise the reference's Python
 *   `total_loss += train_loss.item()`, all_main/pretrain_main.py:79, with no host sync per
 *   step). */
int ctr_step_end_loss(int32_t* step_ctr, const float* loss, double* loss_sum,
                      ctr_stream_t stream);
/* ctr_fm_step_tail: the FM step's dense tail (one process) in one launch —
 *   loss_out[0] = loss_scale * sum(loss_elem[:B]), bias_grad[0] = sum(gz[:B]) (bitwise
 *   ctr_sum_f32), Adam on the flat dense vector (p, g, m, v)[:n] at step ctr[1] (bitwise
 *   ctr_adam_dense; bias_grad may point into g), then ctr_step_end(step_ctr); loss_sum
 *   (may be NULL): loss_sum[0] += (double)loss_out[0], as ctr_step_end_loss.
 *   Replaces: all_main/pretrain_main.py:74-78 (loss.backward's bias gradient, the batch
 *   loss, optimizer.step() on the FM bias) at the end of a step. */
int ctr_fm_step_tail(const float* loss_elem, const float* gz, int64_t B, float loss_scale,
                     float* loss_out, float* bias_grad, float* p, const float* g, float* m,
                     float* v, int64_t n, const float* step_table, int32_t* step_ctr,
                     double beta1, double beta2, double eps, double weight_decay,
                     double* loss_sum, ctr_stream_t stream);

/* ------------------------------------------------ A7: Feature_Embedding -------------
 * out[b] = [ <E[x_bi],E[x_bj]> for i<j in row-major pair order ] ++ flat(E[x_b]),
 * out is [B, F(F-1)/2 + F*K]. Replaces: Feature_embedding.py:51-59. */
int ctr_feature_embedding_forward(const void* idx, int idx_type, int64_t B, int F, int K,
                                  int64_t V, const float* emb, float* out, int32_t* err_flag,
                                  ctr_stream_t stream);
/* ctr_feature_embedding_forward_planes: the same, and the state's three exact bf16 planes
 *   (ctr_planes, >= [B, F(F-1)/2 + F*K]) for the planes GEMM of the policy's first layer
 *   (out_planes NULL: the plain call). Replaces: Feature_embedding.py:51-59 feeding
 *   PG_model.py:52 (the first nn.Linear of Net). */
int ctr_feature_embedding_forward_planes(const void* idx, int idx_type, int64_t B, int F,
                                         int K, int64_t V, const float* emb, float* out,
                                         const ctr_planes* out_planes, int32_t* err_flag,
                                         ctr_stream_t stream);

/* ------------------------------------------ §8f: binary on-disk batches (host) -----
 * ctr_csv_to_bin: the reference's encoded CSV (`label,idx_1..idx_F` per line,
 *   src/encode/data_.py:85; parsed by pd.read_csv at all_main/pretrain_main.py:50-53) ->
 *   a "CTRBIN01" file: 64-byte header (rows, cols = 1+F, max feature id) + int32
 *   [rows][cols] (label, ids), memory-mappable. Streams in constant memory; ragged rows
 *   or non-integer fields fail with the line number. Host code, no GPU needed.
 * ctr_bin_info: header fields of such a file (validates magic and size). */
int ctr_csv_to_bin(const char* csv_path, const char* bin_path, int64_t* rows, int32_t* cols,
                   int64_t* max_id);
int ctr_bin_info(const char* bin_path, int64_t* rows, int32_t* cols, int64_t* max_id,
                 int64_t* data_offset);

/* ------------------------------------- §8f: ensemble prediction + sign reward -------
 * generate_preds of the RL drivers (hybrid_td3_main_per_v10.py:54-164): preds [B, M] (row
 * stride ld_preds; the M pretrained models' pCTRs), actions [B] (ensemble size, 1-based),
 * prob_weights / c_actions [B, M], labels [B] (0/1) -> y_preds [B], rewards [B],
 * return_c_actions [B, M]; M <= 32. Keeps the reference's indexing of the sorted
 * c_actions by the example's ordinal within its action group (line 127). rank_ws:
 * int32[B] scratch. action_type / label_type: CTR_IDX_I32 or CTR_IDX_I64. */
int ctr_ensemble_preds(const float* preds, int64_t B, int M, int64_t ld_preds,
                       const void* actions, int action_type, const float* prob_weights,
                       const float* c_actions, const void* labels, int label_type,
                       float* y_preds, float* rewards, float* return_c_actions, int32_t* rank_ws,
                       ctr_stream_t stream);
/* ctr_ensemble_preds_ex: the same with flags; ctr_ensemble_preds is this with flags = 0.
 *   CTR_ENSEMBLE_TIE_REWARDS: the reward compares with >= (label 1) and <= (label 0), so a tie
 *   with the models' mean earns 1: the base driver's rule (hybrid_td3_main_per.py:114-126).
 *   c_actions NULL: prob_weights take their place (the base driver's generate_preds, lines
 *   56-133, has no c_actions: its softmax runs over the largest prob_weights).
 *   return_c_actions NULL: not computed; rank_ws may then be NULL too. */
enum ctr_ensemble_flags { CTR_ENSEMBLE_TIE_REWARDS = 1 };
int ctr_ensemble_preds_ex(const float* preds, int64_t B, int M, int64_t ld_preds,
                          const void* actions, int action_type, const float* prob_weights,
                          const float* c_actions, const void* labels, int label_type,
                          float* y_preds, float* rewards, float* return_c_actions,
                          int32_t* rank_ws, int flags, ctr_stream_t stream);

/* ------------------------------------------------ §8f: FFM (field-aware FM) ---------
 * tables: a DEVICE array of F pointers, table t = field t's embedding [V, K] (K <= 64,
 * F*V < 2^31). ctr_ffm_forward: z = bias + sum_f lin[x_f] + sum_{i<j} sum_k
 * E_j[x_i,k] * E_i[x_j,k] (p_model.FFM.forward, p_model.py:82-100), with the fused BCE head
 * when labels != NULL (as ctr_fm_forward). ctr_ffm_backward: the F(F-1) row gradients of
 * every example, vals[pos, :] = gz[b] * E_f[x_bt, :] for table t's row x_bf, key[pos] =
 * t*V + x_bf, pos = (b*F + f)*(F-1) + (t < f ? t : t-1) ([B*F*(F-1)] keys, [.., K] vals):
 * a sparse plan over the keys (key range F*V) + ctr_segment_sum_rows give every table's
 * row sums in slot order. */
int ctr_ffm_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                    const float* const* tables, const float* lin, const float* bias, float* z,
                    const float* labels, float mean_div, float* p, float* loss_elem, float* gz,
                    int32_t* err_flag, ctr_stream_t stream);
int ctr_ffm_backward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                     const float* const* tables, const float* gz, int32_t* keys, float* vals,
                     ctr_stream_t stream);
/* ctr_ffm_keys: the keys of ctr_ffm_backward alone (same positions): the table rows an FFM
 * step reads and updates, for the fused trainer's catch-up before the forward. */
int ctr_ffm_keys(const void* idx, int idx_type, int64_t B, int F, int64_t V, int32_t* keys,
                 int32_t* err_flag, ctr_stream_t stream);

/* ------------------------------------------------ §8f: IPNN (InnerPNN) --------------
 * ctr_ipnn_forward: cat[b] = flat(E[x_b]) (F*K) ++ [ <E[x_bi],E[x_bj]> for i<j, row-major ]
 *   (P = F(F-1)/2), cat is [B, >= F*K + P] with row stride ldc: the MLP input of
 *   p_model.InnerPNN.forward (p_model.py:187-195).
 * ctr_ipnn_backward: dslot[b*F+f, :] (slot order, [B*F, K]) = dcat[b, f*K:(f+1)*K]
 *   + sum_{j != f} dcat[b, F*K + pair(f,j)] * E[x_bj, :] — the gradient of every slot's
 *   embedding through the view and the two pair index ops; per-row sums then go through
 *   ctr_segment_sum_rows (embedding_dense_backward of p_model.py:187). */
int ctr_ipnn_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                     const float* emb, float* cat, int64_t ldc, int32_t* err_flag,
                     ctr_stream_t stream);
/* ctr_ipnn_forward_planes: ctr_ipnn_forward writing cat as its three bf16 planes (the
 *   split-bf16 MLP GEMMs' operand) — cat itself may then be NULL (no fp32 copy, no split
 *   pass); with both, both are written. */
int ctr_ipnn_forward_planes(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                            const float* emb, float* cat, int64_t ldc,
                            const ctr_planes* cat_planes, int32_t* err_flag,
                            ctr_stream_t stream);
int ctr_ipnn_backward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                      const float* emb, const float* dcat, int64_t ldd, float* dslot,
                      ctr_stream_t stream);

/* ------------------------------------------------ OPNN (OuterPNN) ---------------------
 * p_model.OuterPNN.forward (p_model.py:244-251). With s[b, :] = sum_f E[x_bf, :] (fp32, in
 * field order) and ksum [K] = kernel.sum(0) of the model's K x K kernel, the reference's
 * cross term sum_i (s_j * kernel[i,j]) * s_j is ksum[j] * s[b,j]^2 (two rounded products).
 * ctr_opnn_forward: cat[b] = flat(E[x_b]) (F*K, bit-exact copies) ++ ksum * s^2 (K), written
 *   as fp32 cat [B, >= F*K + K] (row stride ldc) and / or as its three bf16 planes
 *   (cat_planes, valid region only) — at least one of the two; sum_e [B, K] (optional) = s,
 *   which the backward reads. Ids outside [0, V) read row 0 and raise CTR_EFLAG_INDEX.
 * ctr_opnn_backward: dslot[b*F+f, k] (slot order, [B*F, K]) = dcat[b, f*K+k]
 *   + ((2*ksum[k]) * s[b,k]) * dcat[b, F*K+k] (product rounded before the sum); reads dcat
 *   (row stride ldd), sum_e and ksum only. Per-row sums then go through ctr_segment_sum_rows.
 * Any F >= 1, K >= 1. 16-byte accesses when K % 4 == 0 and the pointers and strides are
 * 16-byte aligned, scalar ones otherwise: the same result either way. B == 0: no launch. */
int ctr_opnn_forward(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                     const float* emb, const float* ksum, float* cat, int64_t ldc,
                     const ctr_planes* cat_planes, float* sum_e, int32_t* err_flag,
                     ctr_stream_t stream);
int ctr_opnn_backward(int64_t B, int F, int K, const float* sum_e, const float* ksum,
                      const float* dcat, int64_t ldd, float* dslot, ctr_stream_t stream);

/* ------------------------------------------------ DCN: the cross network --------------
 * For B examples with x0 = flat(E[x_b]) [D] (row stride ldx), W and bias [L, D] contiguous
 * (the stacked cross_net_w[i].weight and cross_net_b[i]), 1 <= L <= 8:
 *   x_0 = x0;  s_i = <x_i, W_i>;  x_{i+1} = (x0 * s_i + bias_i) + x_i   (that association,
 *   no fma contraction: p_model.py:427-429).
 * ctr_dcn_cross_forward: s [B, L] (all the backward keeps besides x0), and at least one of
 *   xL [B, D] (row stride ldo) = x_L and z [B] = <x_L, w_tail> (needs w_tail [D], the first D
 *   columns of DCN.linear.weight: the cross half of p_model.py:431-433, so that neither x_L
 *   nor cat[x_L, dn] is materialised). x0 is read once; no x_i reaches memory.
 * ctr_dcn_cross_backward: dL/dx_L = gL [B, D] (row stride ldg, optional) + gz[b] * w_tail
 *   (the rank-1 form: gz and w_tail both or neither; at least one form). Outputs dx0 [B, D]
 *   (row stride ldd), dW and dbias [L, D], and dw_tail [D] = sum_b gz[b] * x_L[b] (optional,
 *   rank-1 form only). x0 (and gL) are read once. The batch sums are deterministic: per-block
 *   partials in row order in ws (ctr_dcn_cross_workspace_bytes, independent of B, 16-byte
 *   aligned), added in block order by a second launch; no float atomics. B == 0 zero-fills
 *   dW, dbias and dw_tail.
 * A row's s, x_L, z and dx0 do not depend on B or on the row's position. Vector (16-byte)
 * accesses are used when D, the strides and the pointers allow, scalar ones otherwise. */
int64_t ctr_dcn_cross_workspace_bytes(int64_t B, int D, int L);
int ctr_dcn_cross_forward(int64_t B, int D, int L, const float* x0, int64_t ldx,
                          const float* W, const float* bias, const float* w_tail, float* s,
                          float* xL, int64_t ldo, float* z, ctr_stream_t stream);
int ctr_dcn_cross_backward(int64_t B, int D, int L, const float* x0, int64_t ldx,
                           const float* W, const float* bias, const float* s,
                           const float* gL, int64_t ldg, const float* gz, const float* w_tail,
                           float* dx0, int64_t ldd, float* dW, float* dbias, float* dw_tail,
                           void* ws, int64_t ws_bytes, ctr_stream_t stream);

/* ------------------------------------------------ AFM: pairwise attention -------------
 * p_model.AFM.forward (p_model.py:472-486) up to the pooled vector. Per example b with
 * e_f = E[x_bf] [K] and the pairs p = (i, j), i < j, in row-major order, P = F(F-1)/2:
 *   q_p = e_i * e_j;  h_p = relu(W1 q_p + b1) [A];  s_p = <w2, h_p> + b2[0];
 *   a = softmax_p(s) (max-subtracted);  a'_p = a_p * m1[b,p];  o = sum_p a'_p q_p;  o' = o * m2[b,k]
 * W1 [A, K] = attention_net.weight, b1 [A], w2 [A] = attention_softmax.weight, b2 [1].
 * ctr_afm_forward: pooled [B, K] (row stride ldp) = o'; attn [B, P] (optional) = a, the
 *   softmax BEFORE dropout, the only activation the backward keeps. Ids outside [0, V) read
 *   row 0 and raise CTR_EFLAG_INDEX.
 * ctr_afm_backward: from dpooled = dL/do' [B, K] (row stride ldg) and attn: dslot [B*F, K]
 *   (slot order; per-row sums then go through ctr_segment_sum_rows) and the batch sums dW1
 *   [A, K], db1 [A], dw2 [A], db2 [1]. It gathers e again, recomputes h and takes a from attn:
 *   with do = do' * m2, da_p = m1_p <do, q_p>, c = sum_p a_p da_p, ds_p = a_p (da_p - c),
 *   dh_p = ds_p * w2 * [h_p > 0] (gradient 0 at 0), dq_p = W1^T dh_p + a'_p do,
 *   de_i += dq_p * e_j, de_j += dq_p * e_i; dW1 = sum dh_p (x) q_p, db1 = sum dh_p,
 *   dw2 = sum ds_p h_p, db2 = sum ds_p (zero up to rounding: softmax is shift-invariant).
 * Contracts:
 *   - 2 <= F <= 64, 1 <= K <= 128, 1 <= A <= 128, 0 <= drop_p < 1; anything else, a null
 *     pointer, ldp / ldg < K and a workspace smaller than ctr_afm_workspace_bytes (which does
 *     not depend on B and is a multiple of 16) return CTR_ERR_INVALID before any HIP call.
 *   - B == 0: the forward launches nothing, the backward zero-fills the four batch sums.
 *   - Nothing of size B*P*K or B*P*A reaches global memory: a block stages its example's F
 *     rows once in LDS and forms the pair products from them.
 *   - Any K and A. 16-byte accesses where K and the pointers allow (the gather, W1 in the
 *     backward, dslot), scalar ones otherwise: the same result either way. The K x A product
 *     is plain fp32 FMA.
 *   - Deterministic, no float atomics: a slot's F-1 contributions are added in a fixed
 *     pair order (the rounds of a round-robin schedule); the batch sums are per-block partials in row order in ws, added in block
 *     order by a second launch; two calls on the same inputs give the same bits. Without
 *     dropout (whose counters hold b) a row's pooled, attn and dslot do not depend on B or on
 *     the row's position.
 *   - Dropout: mask element = hash_u32(seed, ctr) >= drop_p*2^32 ? 1/(1-drop_p) : 0 with the
 *     threshold and scale of ctr_gemm_f32 (formed in double from the fp32 drop_p, the
 *     threshold clamped to 2^32 - 1 and truncated); ctr = b*(P+K) + p for m1 and
 *     b*(P+K) + P + k for m2 (uint64). The backward recomputes both from (seed, drop_p).
 *     drop_p == 0: no hash is evaluated.
 * Replaces: p_model.py:473-482 and autograd through them. */
int64_t ctr_afm_workspace_bytes(int64_t B, int F, int K, int A);
int ctr_afm_forward(const void* idx, int idx_type, int64_t B, int F, int K, int A, int64_t V,
                    const float* emb, const float* W1, const float* b1, const float* w2,
                    const float* b2, float drop_p, uint64_t seed, float* pooled, int64_t ldp,
                    float* attn, int32_t* err_flag, ctr_stream_t stream);
int ctr_afm_backward(const void* idx, int idx_type, int64_t B, int F, int K, int A, int64_t V,
                     const float* emb, const float* W1, const float* b1, const float* w2,
                     const float* b2, float drop_p, uint64_t seed, const float* attn,
                     const float* dpooled, int64_t ldg, float* dslot, float* dW1, float* db1,
                     float* dw2, float* db2, void* ws, int64_t ws_bytes, int32_t* err_flag,
                     ctr_stream_t stream);

/* ctr_afm_forward_step / ctr_afm_backward_step: the two entry points above with a dropout seed
 * that advances inside a replayed HIP graph. step_ptr (device int32, may be NULL) is read
 * once by the kernel as t, and
 *   seed_eff = seed + (uint64_t)(uint32_t)t * 0x9E3779B97F4A7C15   (mod 2^64)
 * stands wherever the plain entry points use seed: the call at step t is bit for bit the plain
 * call with seed_eff, which the host can compute. NULL: seed_eff = seed (the plain entry points
 * are these with NULL). Every other contract is the plain entry points'. */
int ctr_afm_forward_step(const void* idx, int idx_type, int64_t B, int F, int K, int A,
                         int64_t V, const float* emb, const float* W1, const float* b1,
                         const float* w2, const float* b2, float drop_p, uint64_t seed,
                         const int32_t* step_ptr, float* pooled, int64_t ldp, float* attn,
                         int32_t* err_flag, ctr_stream_t stream);
int ctr_afm_backward_step(const void* idx, int idx_type, int64_t B, int F, int K, int A,
                          int64_t V, const float* emb, const float* W1, const float* b1,
                          const float* w2, const float* b2, float drop_p, uint64_t seed,
                          const int32_t* step_ptr, const float* attn, const float* dpooled,
                          int64_t ldg, float* dslot, float* dW1, float* db1, float* dw2,
                          float* db2, void* ws, int64_t ws_bytes, int32_t* err_flag,
                          ctr_stream_t stream);

/* ctr_afm_head: AFM's out head for the fused training step (p_model.py:483-486 and the BCE
 * loss), everything between ctr_afm_forward and ctr_afm_backward in one launch. Per example b:
 *   z_lr = bias[0] + (lin[x_b0] + lin[x_b1] + ...)      in the order of ctr_lr_forward
 *   z    = z_lr + (<pooled_b, fc_w> + fc_b[0])          the dot in the order of ctr_deepfm_head
 *   p, loss_elem, gz                                    the BCE head (ctr_bce_sigmoid, mean_div)
 *   dpooled[b, k] = gz[b] * fc_w[k]                     one fp32 multiply
 * z, p, loss_elem and gz are the bits of ctr_deepfm_head(h = pooled, w_out = fc_w, b_out = fc_b,
 * z_fm = the z of ctr_lr_forward, labels, mean_div, drop_scale = 1). The dropout mask of the
 * pooled vector is applied inside ctr_afm_backward, not here.
 * Contracts:
 *   - 2 <= F <= 64, 1 <= K <= 128, V >= 1, mean_div > 0; pooled [B, K] has row stride ldp,
 *     dpooled [B, K] row stride ldg; z, p and loss_elem may be NULL (not written). Anything
 *     else, a null required pointer or ldp / ldg < K returns CTR_ERR_INVALID before any HIP
 *     call. B == 0 launches nothing.
 *   - Ids outside [0, V) read row 0 and raise CTR_EFLAG_INDEX.
 *   - Every access is a 4-byte one: no alignment is asked of any pointer, and none changes a
 *     result. A row's outputs depend on that row alone; no atomics on floats.
 *   - A wave holds 64 / G rows, G = the power of two >= F, at least 16. */
int ctr_afm_head(const void* idx, int idx_type, int64_t B, int F, int K, int64_t V,
                 const float* lin, const float* bias, const float* pooled, int64_t ldp,
                 const float* fc_w, const float* fc_b, const float* labels, float mean_div,
                 float* z, float* p, float* loss_elem, float* gz, float* dpooled, int64_t ldg,
                 int32_t* err_flag, ctr_stream_t stream);

/* ------------------------------------- Prioritized replay memory (hybrid TD3, PER) ------
 * The reference's Memory (Hybrid_TD3_model_PER.py:22-109) with storage and sampling on the
 * device: memory [N, T] and prio [N] (the [N, 1] priority column) are fp32, contiguous, and
 * written in place. No entry point copies to the host or waits for the device. N < 2^31.
 * The priority of a TD error is (|td| + eps)^alpha in fp32 (get_priority).
 * ctr_per_add: rows i = 0 .. n-1 of transitions [n, T] (row stride ldt) go to slot
 *   (start + i) % N in one launch (0 <= start < N; the host never branches on wrap-around):
 *   memory[slot] = transitions[i], prio[slot] = max(prio[slot], priority(td[i])) (a max,
 *   not an overwrite: lines 53, 57, 61). n == 0 is a no-op; n > N is refused (two rows
 *   would share a slot).
 * ctr_per_update: prio[idx[i]] = priority(td[i]) for i < k (batch_update). An index outside
 *   [0, N) is ignored. Duplicate indices are undefined (one of their values is kept), as in
 *   the reference's indexed assignment.
 * ctr_per_keys: the selection keys of elements [0, n_valid), bitwise the ones ctr_per_sample
 *   orders by. An element with p <= 0 or a non-finite p has key -inf (picked last). Otherwise
 *     mode 1 (greedy):      key_i = p_i
 *     mode 0 (stochastic):  key_i = logf(p_i) + G_i, with
 *       h = hash_u32(seed, i) (32 bits, csrc/ctr_common.h), all but its 24 leading
 *       significant bits cleared; v = ((float)h + 0.5f) * 2^-32, exact, in [2^-33, 1 - 2^-24];
 *       E = -log1pf(-v) in [2^-33, 16.7]; G_i = -logf(E) in [-2.9, 22.9] (Gumbel noise, finest
 *       where G is large). Every key of a finite p > 0 is finite; a key of -0 is stored as +0.
 *   The descending order of the top keys is, in distribution, the order of a sequential
 *   weighted draw without replacement (np.random.choice(p=P, replace=False), line 72).
 * ctr_per_sample: the k largest keys of [0, n_valid), 1 <= k <= min(n_valid, 8192), in
 *   descending key order, ties to the lower index (so equal priorities under mode 1 come back
 *   as the lowest slots, in order). Outputs idx [k] (int64), batch [k, T] = memory[idx] and
 *   isw [k] = (prio[idx] / min_p)^(-beta), min_p = the smallest priority of [0, n_valid), also
 *   stored to min_p[0] when given. Radix select over the order-preserving uint32 image of the
 *   keys (computed once into ws, then three streaming passes with integer histograms), a
 *   counting and a compaction pass with index-ordered slots (the ties taken are the lowest
 *   indices), a rank sort in LDS, one gather. No float atomics: the same (prio, seed) gives
 *   the same bits, order included. ws: ctr_per_workspace_bytes(N, k) bytes (4 N + about 100 KB),
 *   16-byte aligned; the size does not depend on the fill level (0 for an N or k out of
 *   range). */
int64_t ctr_per_workspace_bytes(int64_t N, int k);
int ctr_per_add(int64_t N, int T, int64_t start, int64_t n, const float* transitions,
                int64_t ldt, const float* td, float eps, float alpha, float* memory,
                float* prio, ctr_stream_t stream);
/* ctr_per_store_step: the driver's per-batch store in one launch (the two .float() casts, the
 *   cat of five tensors, the ones and ctr_per_add). Row i < n goes to slot (start + i) % N:
 *   memory[slot] = [ (float)idx[i, 0..F) | c_actions[i, 0..A) | d_values[i, 0..A) |
 *   (float)d_action[i] | rewards[i] ], T == F + 2A + 2, and prio[slot] = max(prio[slot],
 *   priority(1.0f)), the expression ctr_per_add evaluates (the same bits). The conversions
 *   round to nearest even (torch's cast). idx [n, F] and d_action [n] are contiguous int32 or
 *   int64; c_actions, d_values and rewards have row strides ldc, ldd (>= A) and ldr (>= 1).
 *   Plain stores, no atomics. n == 0 is a no-op; n > N is refused. */
int ctr_per_store_step(int64_t N, int T, int64_t start, int64_t n, int F, int A, const void* idx,
                       int idx_type, const float* c_actions, int64_t ldc, const float* d_values,
                       int64_t ldd, const void* d_action, int action_type, const float* rewards,
                       int64_t ldr, float eps, float alpha, float* memory, float* prio,
                       ctr_stream_t stream);
int ctr_per_update(int64_t N, int64_t k, const int64_t* idx, const float* td, float eps,
                   float alpha, float* prio, ctr_stream_t stream);
int ctr_per_keys(int64_t n_valid, const float* prio, int mode, uint64_t seed, float* keys,
                 ctr_stream_t stream);
int ctr_per_sample(int64_t N, int T, int64_t n_valid, int k, int mode, uint64_t seed,
                   float beta, const float* memory, const float* prio, int64_t* idx,
                   float* batch, float* isw, float* min_p, void* ws, int64_t ws_bytes,
                   ctr_stream_t stream);

/* ---------------------------------- Evaluation metrics: exact ROC AUC, BCE loss, rewards --
 * What the drivers' test() computes on the host (sklearn's roc_auc_score over .tolist()ed
 * predictions, a .item() per batch loss, torch.sum(rewards).item()), kept on the device with
 * no host read: batches are appended to a record buffer, and one call sorts and reduces it.
 * records [cap] (8-byte words), the workspace (ctr_metrics_workspace_bytes(cap), 16-byte
 * aligned) and the state block (CTR_METRICS_STATE_BYTES, 8-byte aligned) are caller-owned
 * device memory; 1 <= cap < 2^31. The state block is sixteen 8-byte words:
 *   [0] U2, [1] P, [2] N (uint64)     written by ctr_metrics_auc
 *   [3] loss_sum (fp64)               sum over loss batches of (batch BCE sum / batch size)
 *   [4] nll_sum (fp64)                sum of every example's BCE
 *   [5] reward_sum (fp64)
 *   [6] batches, [7] loss_count (int64)   appends with the loss, and their examples
 *   [8] low 32 bits: CTR_METRICS_FLAG_* bits (int32); the rest is reserved (zero)
 * ctr_metrics_reset zeroes it (one memset on the stream).
 * ctr_metrics_append: example i < n (prediction pred[i * stride], stride >= 1 in elements;
 *   label labels[i], contiguous, of type CTR_LABEL_*; reward rewards[i], optional) becomes
 *   records[offset + i] = (key << 1) | label, key the order-preserving uint32 image of the
 *   fp32 bits of pred + 0.0f (so -0.0 and +0.0 tie, as they do in sklearn). The host passes the
 *   offset: there is no device counter. With with_loss != 0 the batch's BCE
 *   -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) (log in double of the fp32 p) is
 *   summed in fp64 and words [3], [4], [6], [7] advance; rewards advance word [5]. One launch
 *   for n <= 16384, two above; every sum in an order fixed by n, no floating-point atomics: the
 *   same inputs give the same bits. A NaN prediction, a label other than 0/1, and with the loss
 *   a prediction outside [0, 1] OR their flag into word [8] and add nothing to the loss; nothing
 *   faults and nothing outside records[offset, offset + n) is written. n == 0: no launch.
 * ctr_metrics_auc: sorts records[0, count) by their low 33 bits in place (stable LSD radix
 *   sort, two launches per pass, the workspace holds the second buffer) and writes
 *   P = positives, N = negatives, U2 = sum over positives of (2 * negatives with a smaller
 *   prediction + negatives with an equal one), all exact integers:
 *   AUC = U2 / (2 P N), one division left to the host. count == 0: no launch.
 * ctr_metrics_tile: records per sort / reduce tile (the sizes around which tests probe). */
#define CTR_METRICS_STATE_BYTES 128
enum ctr_label_type { CTR_LABEL_F32 = 0, CTR_LABEL_I32 = 1, CTR_LABEL_I64 = 2 };
enum ctr_metrics_flag {
  CTR_METRICS_FLAG_NAN = 1,    /* a NaN prediction */
  CTR_METRICS_FLAG_LABEL = 2,  /* a label other than 0 / 1 */
  CTR_METRICS_FLAG_RANGE = 4   /* a prediction outside [0, 1] while the loss was asked for */
};
int ctr_metrics_tile(void);
int64_t ctr_metrics_workspace_bytes(int64_t cap);
int ctr_metrics_reset(void* state, ctr_stream_t stream);
int ctr_metrics_append(int64_t cap, int64_t offset, int64_t n, const float* pred,
                       int64_t stride, const void* labels, int label_type,
                       const float* rewards, int with_loss, uint64_t* records, void* ws,
                       int64_t ws_bytes, void* state, ctr_stream_t stream);
int ctr_metrics_auc(int64_t cap, int64_t count, uint64_t* records, void* ws, int64_t ws_bytes,
                    void* state, ctr_stream_t stream);

/* ------------------------------------------- Hybrid TD3 agent (actor, twin critics) -----
 * The small kernels of Critic, hybrid_actors and Hybrid_TD3_Model.learn
 * (Hybrid_TD3_model_PER.py:111-393); the Linear layers run on ctr_gemm_f32_ex. All fp32, no
 * float atomics, every sum in an order fixed by the sizes: the same inputs give the same bits.
 * ctr_bn_forward, ctr_bn_backward and ctr_soft_update_multi use 16-byte accesses when N (or
 * numel), every row stride and every pointer allow them and scalar ones otherwise; the noise,
 * action-head, smoothing and critic-loss kernels (A <= 64 columns, [B] vectors) are scalar.
 * B < 2^31.
 * ctr_bn_forward: nn.BatchNorm1d on x [B, N] (row stride ldx) -> y (row stride ldy, so y may
 *   be a column block of a wider matrix), then ReLU when relu != 0.
 *   training != 0: per-column mean and biased variance over the B >= 2 rows (B < 2 is refused,
 *     as torch refuses it), two passes with fp64 accumulators, never E[x^2] - E[x]^2;
 *     invstd = 1 / sqrt(var + eps); y = (x - mean) * invstd * gamma + beta, evaluated in fp64
 *     and rounded once. save_mean, save_invstd [N] (optional) are what ctr_bn_backward needs;
 *     save_mean_lo, save_invstd_lo [N] (optional) are the parts of the fp64 mean and invstd
 *     that their fp32 values drop (with few rows dx's terms cancel almost entirely, and the
 *     backward, given them, loses nothing to that rounding). running_mean / running_var (both or neither) are updated in
 *     place: rm = (1 - momentum) * rm + momentum * mean, rv likewise with the unbiased
 *     variance var * B / (B - 1).
 *   training == 0: y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta, row-local,
 *     any B >= 1; nothing but y is written.
 * ctr_bn_backward: the training-mode backward from dy (row stride lddy), x and the saved
 *   statistics. With relu != 0, dy is first masked by y > 0 (y: the forward's output, row
 *   stride ldy). dbeta = sum g, dgamma = sum g * x_hat, and, unless dx is NULL,
 *   dx = gamma * invstd * (g - dbeta / B - x_hat * dgamma / B) (row stride ldd), in one launch,
 *   in fp64 rounded once; save_mean_lo and save_invstd_lo may be NULL (taken as 0).
 *   The eval-mode backward is not provided.
 * ctr_td3_noise: out[i] = z(seed, offset + i), i < n, unit normal by Box-Muller from a
 *   stateless hash: h1 = hash_u32(seed, 2e), h2 = hash_u32(seed, 2e + 1) (csrc/ctr_common.h),
 *   u = ((float)(h >> 8) + 0.5f) * 2^-24 in (0, 1), z = sqrtf(-2 logf(u1)) * cosf(2 pi u2),
 *   |z| < 5.9. ctr_td3_act and ctr_td3_smooth in noise_mode 2 use element B * A * head + row *
 *   A + col of stream `seed` (head 0: continuous, 1: discrete) through the same device
 *   function: ctr_td3_noise(B * A, seed, head * B * A) returns the bits they consumed.
 * ctr_td3_act: the two action heads of hybrid_actors from their pre-activations pre_c, pre_d
 *   [B, A] (row stride ldp), A <= 64. c = tanh(pre_c), d = tanh(pre_d); with noise_mode 1
 *   (noise_c, noise_d [B, A] contiguous) or 2 (seed), v = clamp(v + noise * sigma, -1, 1)
 *   (lines 234, 238); noise_mode 0 is tanh only (evaluate). Outputs c_actions, d_actions
 *   [B, A], and optionally c_softmax = softmax(c_actions) [B, A] and d_index [B] (int64) =
 *   argmax(d_actions) + 1, the LOWEST index among equal values (argsort(-d)[:, 0] + 1).
 * ctr_td3_smooth: target policy smoothing (lines 354-355) of both heads:
 *   out = clamp(mean + clamp(0.2 * noise, -0.5, 0.5), -1, 1), mean [B, A] (row stride ldm;
 *   apply_tanh != 0: the means are pre-activations, tanh is applied first), out with row stride
 *   ldo: two column blocks of the target critic's input. noise_mode 1 or 2 as above.
 * ctr_td3_critic_loss: from q1, q2, q1_t, q2_t, isw [B] and r (stride ldr: a column of the
 *   sampled batch): q_target = r + gamma * min(q1_t, q2_t); td = 2 q_target - q1 - q2;
 *   loss[0] = mean(isw * ((q1 - q_target)^2 + (q2 - q_target)^2)); dq = 2 isw (q - q_target) / B.
 *   One block, fixed order.
 * ctr_soft_update_multi: target = target * (1 - tau) + source * tau for `count` (<= 4096)
 *   tensors in one launch; table is a DEVICE array of count entries, max_numel the largest
 *   numel in it (it sizes the grid). (float)(1.0 - tau) and (float)tau multiply in fp32, each
 *   product rounded before the sum, as line 335 evaluates. */
typedef struct ctr_soft_update_entry {
  float* target; const float* source; int64_t numel;
} ctr_soft_update_entry;
int ctr_bn_forward(int64_t B, int N, const float* x, int64_t ldx, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float eps,
                   float momentum, int training, int relu, float* y, int64_t ldy,
                   float* save_mean, float* save_mean_lo, float* save_invstd,
                   float* save_invstd_lo, ctr_stream_t stream);
int ctr_bn_backward(int64_t B, int N, const float* dy, int64_t lddy, const float* y,
                    int64_t ldy, int relu, const float* x, int64_t ldx, const float* save_mean,
                    const float* save_mean_lo, const float* save_invstd,
                    const float* save_invstd_lo, const float* gamma, float* dgamma, float* dbeta,
                    float* dx, int64_t ldd, ctr_stream_t stream);
int ctr_td3_noise(int64_t n, uint64_t seed, uint64_t offset, float* out, ctr_stream_t stream);
int ctr_td3_act(int64_t B, int A, const float* pre_c, const float* pre_d, int64_t ldp,
                int noise_mode, const float* noise_c, const float* noise_d, uint64_t seed,
                float sigma, float* c_actions, float* c_softmax, float* d_actions,
                int64_t* d_index, ctr_stream_t stream);
int ctr_td3_smooth(int64_t B, int A, const float* mean_c, const float* mean_d, int64_t ldm,
                   int apply_tanh, int noise_mode, const float* noise_c, const float* noise_d,
                   uint64_t seed, float* out_c, float* out_d, int64_t ldo, ctr_stream_t stream);
int ctr_td3_critic_loss(int64_t B, const float* q1, const float* q2, const float* q1_t,
                        const float* q2_t, const float* r, int64_t ldr, const float* isw,
                        float gamma, float* q_target, float* td, float* loss, float* dq1,
                        float* dq2, ctr_stream_t stream);
int ctr_soft_update_multi(int count, const ctr_soft_update_entry* table, int64_t max_numel,
                          double tau, ctr_stream_t stream);

/* ------------------------------------------- v10 hybrid TD3 agent (csrc/td3_v10.hip) -----
 * The small kernels of v10_Hybrid_TD3_model_PER.py. All fp32 with A <= 64 columns; a row takes
 * the next power of two >= A lanes of a wave. Sums that cross blocks leave one partial per
 * block in an order fixed by the sizes, and the next launch combines them in that order: the
 * same inputs give the same bits. B < 2^31.
 * ctr_td3v10_uniform: out[i] = u(seed, offset + i) in (0, 1), i < n:
 *   u = ((float)(hash_u32(seed, 2 e) >> 8) + 0.5f) * 2^-24, the first uniform of
 *   ctr_td3_noise's element e (take uniforms and normals of one seed from disjoint ranges).
 * ctr_td3v10_heads: the action heads from the pre-activations pre_c, pre_d [B, A] (row stride
 *   ldp), the unit normals noise_c, noise_d and the uniforms `uniform` (all [B, A] contiguous).
 *   g = -log(-log(u + 1e-20) + 1e-20). By mode:
 *     0 act:    c_means = tanh(pre_c); c_softmax = softmax(c + (0.2 n_c + c));
 *               d_action = softmax(((d_q + (0.2 n_d + d_q)) + g) / temperature)   (lines 229-246)
 *     1 plain:  c_means = tanh(pre_c); c_softmax = softmax(c_means);
 *               d_action = softmax((d_q + g) / temperature)                       (line 526)
 *     2 random: c_means = clamp(n_c, -1, 1); c_softmax = softmax(c_means);
 *               d_action = softmax(n_d); pre_c, pre_d, uniform unused             (lines 395-402)
 *     3 best:   c_means = tanh(pre_c); c_softmax = softmax(c_means); d_action is not written
 *               and d_index = argmax(d_q + g) + 1                                 (lines 410-421)
 *   d_index [B] (int64) = argmax(d_action) + 1, the LOWEST index among equal values.
 *   c_softmax, d_action and d_index are optional.
 * ctr_td3v10_rank_mask: to_next_state_c_actions / to_current_state_c_actions (lines 427-472)
 *   without their loops. choose = argmax(d[b]) + 1 (lowest index among equal values); the rank
 *   of column m is #{j: c_j > c_m} + #{j < m: c_j == c_m}; it is kept when rank < choose.
 *   out_c[b, m] = kept ? clamp(v, -1, 1) : 0 with v = c + (0.2 noise + c) when noise ([B, A]
 *   contiguous) is given, else c. d, c, out_c have row strides ldd, ldc, ldo; out_d (optional,
 *   row stride ldo) receives a copy of d and keep (optional, [B, A] bytes) the mask: out_c and
 *   out_d are the two action column blocks of a critic's input.
 * ctr_td3v10_heads_backward: the actor loss's gradient at the heads' pre-activations from the
 *   critic-input gradients g_c, g_d [B, A] (row stride ldg) of the c and d columns:
 *   d_pre_c = ((keep ? g_c : 0) + reg 2 c / (B A)) (1 - c^2)  (mask, the clamp, which is the
 *   identity on tanh's range, the regulariser reg * mean(c^2), tanh');
 *   d_d_q = p (g_d - sum_j p_j g_d_j) / temperature + reg 2 d_q / (B A) with p = d_soft, the
 *   softmax at `temperature`, and the regulariser reg * mean(d_q^2). The argmax and the rank
 *   carry no gradient. c_means, d_soft, d_pre_c, d_d_q: [B, A] contiguous; d_q: row stride ldq.
 * ctr_grad_sumsq, ctr_grad_clip_scale: torch's clip_grad_norm_ over `count` (<= 64) tensors.
 *   table is a HOST array (it travels in the kernel arguments: gradients are new tensors at
 *   every step and nothing is copied to the device for them); max_numel is the largest numel.
 *   ctr_grad_sumsq leaves min(16, ceil(max_numel / 2048)) fp64 partial sums of squares per
 *   tensor in ws (ctr_grad_clip_workspace_bytes(count) bytes, 8-byte aligned), each added in an
 *   order fixed by the sizes. ctr_grad_clip_scale, given the same table and ws, adds the
 *   partials in one fixed order in every block, norm = (float)sqrt(sum), writes it to norm_out
 *   (a device scalar, optional) and multiplies every element by
 *   min(1, max_norm / (norm + 1e-6)) in fp32.
 * ctr_td3v10_store: rows i < n of transitions [n, T] (row stride ldt) go to slot
 *   (start + i) % N of memory [N, T], n <= N; the slot's two priorities are OVERWRITTEN by
 *   td2[i] ([n, 2] contiguous, Memory.add: one launch) or, when td2 is NULL, by
 *   (seed, transitions[i, T-1]) with seed = 1 when the max of the WHOLE prio2 [N, 2] (both
 *   columns, every row, taken before any row is written) is 0, else that max (store_transition,
 *   lines 350-356). That form is two launches: per-block maxima into ws
 *   (CTR_TD3V10_MAX_WS_BYTES, needed only here), which every block of the store launch
 *   reduces; nothing returns to the host. seed_out (optional) receives seed.
 * ctr_td3v10_sample: ctr_per_sample's stochastic select (the same kernels, workspace and key
 *   formula) on the v10 memory: the priority of row i < n_valid is (|prio2[i, 0]| + eps)^alpha,
 *   evaluated where the select, the minimum and isw = (p / min p)^(-beta) read it. Nothing is
 *   written to prio2. ws: ctr_per_workspace_bytes(N, k).
 * ctr_td3v10_keys: the selection keys of rows [0, n_valid), bitwise the ones ctr_td3v10_sample
 *   orders by for `seed` (ctr_per_keys on the transformed priorities).
 * ctr_td3v10_update: prio2[idx[i], 0] = td[i], i < k (the raw signed error; column 1 is not
 *   touched; an index outside [0, N) is skipped).
 * ctr_bn_eval_backward: the parameter gradients of an eval-mode BatchNorm1d,
 *   dbeta = sum dy, dgamma = sum dy (x - running_mean) / sqrt(running_var + eps), over the B
 *   rows in fp64 in a fixed order; no dx. */
#define CTR_GRAD_CLIP_MAX_TENSORS 64
#define CTR_TD3V10_MAX_WS_BYTES 4096
typedef struct ctr_grad_entry {
  float* grad; int64_t numel;
} ctr_grad_entry;
int ctr_td3v10_uniform(int64_t n, uint64_t seed, uint64_t offset, float* out,
                       ctr_stream_t stream);
int ctr_td3v10_heads(int64_t B, int A, int mode, const float* pre_c, const float* pre_d,
                     int64_t ldp, const float* noise_c, const float* noise_d,
                     const float* uniform, float temperature, float* c_means, float* c_softmax,
                     float* d_action, int64_t* d_index, ctr_stream_t stream);
int ctr_td3v10_rank_mask(int64_t B, int A, const float* d, int64_t ldd, const float* c,
                         int64_t ldc, const float* noise, float* out_c, float* out_d, int64_t ldo,
                         uint8_t* keep, ctr_stream_t stream);
int ctr_td3v10_heads_backward(int64_t B, int A, const float* g_c, const float* g_d, int64_t ldg,
                              const uint8_t* keep, const float* c_means, const float* d_q,
                              int64_t ldq, const float* d_soft, float temperature, float reg,
                              float* d_pre_c, float* d_d_q, ctr_stream_t stream);
int64_t ctr_grad_clip_workspace_bytes(int count);
int ctr_grad_sumsq(int count, const ctr_grad_entry* table, int64_t max_numel, void* ws,
                   int64_t ws_bytes, ctr_stream_t stream);
int ctr_grad_clip_scale(int count, const ctr_grad_entry* table, int64_t max_numel, float max_norm,
                        const void* ws, int64_t ws_bytes, float* norm_out, ctr_stream_t stream);
int ctr_td3v10_store(int64_t N, int T, int64_t start, int64_t n, const float* transitions,
                     int64_t ldt, const float* td2, void* ws, int64_t ws_bytes,
                     float* memory, float* prio2, float* seed_out, ctr_stream_t stream);
int ctr_td3v10_keys(int64_t n_valid, const float* prio2, float eps, float alpha, uint64_t seed,
                    float* keys, ctr_stream_t stream);
int ctr_td3v10_sample(int64_t N, int T, int64_t n_valid, int k, uint64_t seed, float beta,
                      float eps, float alpha, const float* memory, const float* prio2,
                      int64_t* idx, float* batch, float* isw, float* min_p, void* ws,
                      int64_t ws_bytes, ctr_stream_t stream);
int ctr_td3v10_update(int64_t N, int64_t k, const int64_t* idx, const float* td, float* prio2,
                      ctr_stream_t stream);
int ctr_bn_eval_backward(int64_t B, int N, const float* dy, int64_t lddy, const float* x,
                         int64_t ldx, const float* running_mean, const float* running_var,
                         float eps, float* dgamma, float* dbeta, ctr_stream_t stream);

/* ------------------------------------------------------ A8: REINFORCE (PG) -----------
 * ctr_softmax_rows: out[b,:] = softmax(x[b,:]) (PG_model.py:56).
 * ctr_pg_discount_norm: discounted return of an episode, reverse recurrence
 *   d[i] = r[i] + gamma*d[i+1] in fp64, then (d - mean)/std (population std), written as
 *   fp64 `out` and fp32 `out_f32`; stats[0..1] = mean, std (fp64, std before division).
 *   Replaces PG_model.py:139-154.
 * ctr_pg_loss_grad: loss = sum_b(-log probs[b, act_b - 1]) * mean(vt) (PG_model.py:104-107,
 *   actions 1-based) and the gradient w.r.t. the softmax LOGITS (softmax backward fused),
 *   scaled by grad_scale. loss_out is a device scalar.
 * ctr_pg_vt_mean: out[0] = mean(vt[0..n)) summed in the order ctr_pg_loss_grad uses.
 * ctr_pg_loss_grad_global: ctr_pg_loss_grad for one rank's slice of an episode that is
 *   split over data-parallel ranks: c = vt_mean[0] (the episode-wide mean, device scalar)
 *   and loss_out = sum_b(-log probs[b, act_b - 1]) * vt_mean[0], this rank's share of the
 *   episode loss (the shares sum to it). Same reference lines as ctr_pg_loss_grad. */
int ctr_softmax_rows(const float* x, int64_t B, int A, float* out, ctr_stream_t stream);
int64_t ctr_pg_workspace_bytes(int64_t n);
int ctr_pg_discount_norm(const float* r, int64_t n, double gamma, double* out, float* out_f32,
                         double* stats, void* ws, int64_t ws_bytes, ctr_stream_t stream);
int ctr_pg_loss_grad(const float* probs, const int64_t* acts, const float* vt, int64_t B,
                     int A, float grad_scale, float* loss_out, float* dlogits, void* ws,
                     int64_t ws_bytes, ctr_stream_t stream);
int ctr_pg_vt_mean(const float* vt, int64_t n, float* out, ctr_stream_t stream);
int ctr_pg_loss_grad_global(const float* probs, const int64_t* acts, int64_t B, int A,
                            const float* vt_mean, float grad_scale, float* loss_out,
                            float* dlogits, ctr_stream_t stream);


/* ==== Op-level interface: one POD argument struct per torch.library op ====
 * ctr_op_<op>(const ctr_<op>_args* a, stream) is the C form of the `ctr::<op>` PyTorch op
 * (rl_ctr_prediction_amd/torch_ops.py) — what a binding without torch (ctypes, cgo, JNI)
 * calls. Each composes the entry points above with the same results, bit for bit. (The
 * `ctr_op_` prefix keeps the names apart from the flat entry points: C has no overloads.)
 * Scratch: ctr_workspace_bytes(op, dims, n_dims) with the op's dims listed below; the op
 * carves its plan / partials / row map out of `ws`. Outputs that the reference returns as
 * fresh tensors (dense gradients) are caller-owned buffers the op zero-fills itself.
 * `flags`: CTR_OPF_DETERMINISTIC (every op here is deterministic: sums in a fixed order, no
 * float atomics; the flag is accepted and always honoured). */
enum ctr_op {
  CTR_OP_FM_FWD = 1,               /* dims: none                     */
  CTR_OP_FM_BWD = 2,               /* dims: {B, F, K, V}             */
  CTR_OP_DEEPFM_GATHER_CONCAT = 3, /* dims: none                     */
  CTR_OP_EMB_SCATTER_ADD = 4,      /* dims: {n_slots, K, V}          */
  CTR_OP_ADAM_DENSE = 5,           /* dims: none                     */
  CTR_OP_ADAM_ROWWISE = 6,         /* dims: {V}                      */
  CTR_OP_PAIRWISE_FE = 7,          /* dims: none                     */
  CTR_OP_PG_RETURNS = 8            /* dims: {n}                      */
};
enum ctr_op_flags { CTR_OPF_DETERMINISTIC = 1 };
/* Scratch bytes of op `op` for `dims` (see enum ctr_op); -1 for an unknown op or bad dims. */
int64_t ctr_workspace_bytes(int op, const int64_t* dims, int n_dims);

/* ctr::fm_fwd — FM.forward logit and the per-example embedding sums its backward needs:
 * z[B] (the [B,1] logit), sum_e[B,K]. Replaces p_model.py:40-57. */
typedef struct ctr_fm_fwd_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* emb; const float* lin; const float* bias;
  float* z; float* sum_e; int32_t* err_flag; int flags;
} ctr_fm_fwd_args;
int ctr_op_fm_fwd(const ctr_fm_fwd_args* a, ctr_stream_t stream);

/* ctr::fm_bwd — FM's parameter gradients from dL/dz: dense g_emb[V,K], g_lin[V] (both
 * zero-filled here, then the batch's rows written: embedding_dense_backward) and g_bias[1]
 * = sum gz. Replaces autograd through p_model.py:40-57 (all_main/pretrain_main.py:77). */
typedef struct ctr_fm_bwd_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* emb; const float* sum_e; const float* gz;
  float* g_emb; float* g_lin; float* g_bias;
  void* ws; int64_t ws_bytes; int32_t* err_flag; int flags;
} ctr_fm_bwd_args;
int ctr_op_fm_bwd(const ctr_fm_bwd_args* a, ctr_stream_t stream);

/* ctr::deepfm_gather_concat — out[B, F*K] = E[x] flattened (DeepFM's MLP input,
 * p_model.py:320-321). */
typedef struct ctr_deepfm_gather_concat_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* emb; float* out; int32_t* err_flag; int flags;
} ctr_deepfm_gather_concat_args;
int ctr_op_deepfm_gather_concat(const ctr_deepfm_gather_concat_args* a, ctr_stream_t stream);

/* ctr::emb_scatter_add — dense[V,K] (zero-filled here) = embedding_dense_backward of
 * per-slot gradients grad_slots[n_slots, K] at ids idx[n_slots] (slot order kept per row). */
typedef struct ctr_emb_scatter_add_args {
  const void* idx; int idx_type; int64_t n_slots; int K; int64_t V;
  const float* grad_slots; float* dense;
  void* ws; int64_t ws_bytes; int32_t* err_flag; int flags;
} ctr_emb_scatter_add_args;
int ctr_op_emb_scatter_add(const ctr_emb_scatter_add_args* a, ctr_stream_t stream);

/* ctr::adam_dense — one torch.optim.Adam step (coupled L2) of n elements at step `step`
 * (1-based; the bias corrections are computed here in double as torch does). Replaces
 * all_main/pretrain_main.py:78 (optimizer.step) for dense parameters. */
typedef struct ctr_adam_dense_args {
  float* p; const float* g; float* m; float* v; int64_t n; int64_t step;
  double lr; double beta1; double beta2; double eps; double weight_decay; int flags;
} ctr_adam_dense_args;
int ctr_op_adam_dense(const ctr_adam_dense_args* a, ctr_stream_t stream);

/* ctr::adam_rowwise — the same Adam step for EVERY row of emb[V,K] (dense semantics), the
 * gradient of row rows[u] being grad_rows[u,:] and 0 for rows not listed (rows distinct).
 * A listed row outside [0, V) is not applied and raises CTR_EFLAG_INDEX in *err_flag (may
 * be NULL: then such a row is dropped silently), as the torch op's index_copy_ raises. */
typedef struct ctr_adam_rowwise_args {
  float* emb; float* m; float* v; int64_t V; int K;
  const void* rows; int rows_type; int64_t n_rows; const float* grad_rows; int64_t step;
  double lr; double beta1; double beta2; double eps; double weight_decay;
  void* ws; int64_t ws_bytes; int32_t* err_flag; int flags;
} ctr_adam_rowwise_args;
int ctr_op_adam_rowwise(const ctr_adam_rowwise_args* a, ctr_stream_t stream);

/* ctr::pairwise_fe — Feature_Embedding.forward: [B, F(F-1)/2 + F*K]
 * (Feature_embedding.py:51-59). */
typedef struct ctr_pairwise_fe_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* emb; float* out; int32_t* err_flag; int flags;
} ctr_pairwise_fe_args;
int ctr_op_pairwise_fe(const ctr_pairwise_fe_args* a, ctr_stream_t stream);

/* ctr::pg_returns — discount_and_norm_rewards: vt (fp64) and its fp32 copy
 * (PG_model.py:139-154). */
typedef struct ctr_pg_returns_args {
  const float* r; int64_t n; double gamma; double* vt; float* vt_f32;
  void* ws; int64_t ws_bytes; int flags;
} ctr_pg_returns_args;
int ctr_op_pg_returns(const ctr_pg_returns_args* a, ctr_stream_t stream);

/* The hybrid TD3 agent's operations in struct form: each forwards its fields to the flat entry
 * point of the same name (see there for the semantics). None needs scratch. */
typedef struct ctr_bn_forward_args {
  int64_t B; int N; const float* x; int64_t ldx; const float* gamma; const float* beta;
  float* running_mean; float* running_var; float eps; float momentum; int training; int relu;
  float* y; int64_t ldy; float* save_mean; float* save_mean_lo; float* save_invstd;
  float* save_invstd_lo;
} ctr_bn_forward_args;
int ctr_op_bn_forward(const ctr_bn_forward_args* a, ctr_stream_t stream);

typedef struct ctr_bn_backward_args {
  int64_t B; int N; const float* dy; int64_t lddy; const float* y; int64_t ldy; int relu;
  const float* x; int64_t ldx; const float* save_mean; const float* save_mean_lo;
  const float* save_invstd; const float* save_invstd_lo; const float* gamma; float* dgamma;
  float* dbeta; float* dx; int64_t ldd;
} ctr_bn_backward_args;
int ctr_op_bn_backward(const ctr_bn_backward_args* a, ctr_stream_t stream);

typedef struct ctr_td3_noise_args {
  int64_t n; uint64_t seed; uint64_t offset; float* out;
} ctr_td3_noise_args;
int ctr_op_td3_noise(const ctr_td3_noise_args* a, ctr_stream_t stream);

typedef struct ctr_td3_act_args {
  int64_t B; int A; const float* pre_c; const float* pre_d; int64_t ldp; int noise_mode;
  const float* noise_c; const float* noise_d; uint64_t seed; float sigma;
  float* c_actions; float* c_softmax; float* d_actions; int64_t* d_index;
} ctr_td3_act_args;
int ctr_op_td3_act(const ctr_td3_act_args* a, ctr_stream_t stream);

typedef struct ctr_td3_smooth_args {
  int64_t B; int A; const float* mean_c; const float* mean_d; int64_t ldm; int apply_tanh;
  int noise_mode; const float* noise_c; const float* noise_d; uint64_t seed;
  float* out_c; float* out_d; int64_t ldo;
} ctr_td3_smooth_args;
int ctr_op_td3_smooth(const ctr_td3_smooth_args* a, ctr_stream_t stream);

typedef struct ctr_td3_critic_loss_args {
  int64_t B; const float* q1; const float* q2; const float* q1_t; const float* q2_t;
  const float* r; int64_t ldr; const float* isw; float gamma;
  float* q_target; float* td; float* loss; float* dq1; float* dq2;
} ctr_td3_critic_loss_args;
int ctr_op_td3_critic_loss(const ctr_td3_critic_loss_args* a, ctr_stream_t stream);

typedef struct ctr_soft_update_multi_args {
  int count; const ctr_soft_update_entry* table; int64_t max_numel; double tau;
} ctr_soft_update_multi_args;
int ctr_op_soft_update_multi(const ctr_soft_update_multi_args* a, ctr_stream_t stream);

/* The v10 agent's operations in struct form, each forwarding to its flat entry point. */
typedef struct ctr_td3v10_uniform_args {
  int64_t n; uint64_t seed; uint64_t offset; float* out;
} ctr_td3v10_uniform_args;
int ctr_op_td3v10_uniform(const ctr_td3v10_uniform_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_heads_args {
  int64_t B; int A; int mode; const float* pre_c; const float* pre_d; int64_t ldp;
  const float* noise_c; const float* noise_d; const float* uniform; float temperature;
  float* c_means; float* c_softmax; float* d_action; int64_t* d_index;
} ctr_td3v10_heads_args;
int ctr_op_td3v10_heads(const ctr_td3v10_heads_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_rank_mask_args {
  int64_t B; int A; const float* d; int64_t ldd; const float* c; int64_t ldc; const float* noise;
  float* out_c; float* out_d; int64_t ldo; uint8_t* keep;
} ctr_td3v10_rank_mask_args;
int ctr_op_td3v10_rank_mask(const ctr_td3v10_rank_mask_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_heads_backward_args {
  int64_t B; int A; const float* g_c; const float* g_d; int64_t ldg; const uint8_t* keep;
  const float* c_means; const float* d_q; int64_t ldq; const float* d_soft; float temperature;
  float reg; float* d_pre_c; float* d_d_q;
} ctr_td3v10_heads_backward_args;
int ctr_op_td3v10_heads_backward(const ctr_td3v10_heads_backward_args* a, ctr_stream_t stream);

typedef struct ctr_grad_sumsq_args {
  int count; const ctr_grad_entry* table; int64_t max_numel; void* ws; int64_t ws_bytes;
} ctr_grad_sumsq_args;
int ctr_op_grad_sumsq(const ctr_grad_sumsq_args* a, ctr_stream_t stream);

typedef struct ctr_grad_clip_scale_args {
  int count; const ctr_grad_entry* table; int64_t max_numel; float max_norm; const void* ws;
  int64_t ws_bytes; float* norm_out;
} ctr_grad_clip_scale_args;
int ctr_op_grad_clip_scale(const ctr_grad_clip_scale_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_store_args {
  int64_t N; int T; int64_t start; int64_t n; const float* transitions; int64_t ldt;
  const float* td2; void* ws; int64_t ws_bytes; float* memory; float* prio2;
  float* seed_out;
} ctr_td3v10_store_args;
int ctr_op_td3v10_store(const ctr_td3v10_store_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_keys_args {
  int64_t n_valid; const float* prio2; float eps; float alpha; uint64_t seed; float* keys;
} ctr_td3v10_keys_args;
int ctr_op_td3v10_keys(const ctr_td3v10_keys_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_sample_args {
  int64_t N; int T; int64_t n_valid; int k; uint64_t seed; float beta; float eps; float alpha;
  const float* memory; const float* prio2; int64_t* idx; float* batch; float* isw; float* min_p;
  void* ws; int64_t ws_bytes;
} ctr_td3v10_sample_args;
int ctr_op_td3v10_sample(const ctr_td3v10_sample_args* a, ctr_stream_t stream);

typedef struct ctr_td3v10_update_args {
  int64_t N; int64_t k; const int64_t* idx; const float* td; float* prio2;
} ctr_td3v10_update_args;
int ctr_op_td3v10_update(const ctr_td3v10_update_args* a, ctr_stream_t stream);

typedef struct ctr_bn_eval_backward_args {
  int64_t B; int N; const float* dy; int64_t lddy; const float* x; int64_t ldx;
  const float* running_mean; const float* running_var; float eps; float* dgamma; float* dbeta;
} ctr_bn_eval_backward_args;
int ctr_op_bn_eval_backward(const ctr_bn_eval_backward_args* a, ctr_stream_t stream);

/* ctr::afm_pool — ctr_afm_forward / ctr_afm_backward with their arguments in a struct (the
 * flat entry points' contract; ws sized by ctr_afm_workspace_bytes). */
typedef struct ctr_afm_fwd_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int A; int64_t V;
  const float* emb; const float* W1; const float* b1; const float* w2; const float* b2;
  float drop_p; uint64_t seed; float* pooled; int64_t ldp; float* attn; int32_t* err_flag;
} ctr_afm_fwd_args;
int ctr_op_afm_fwd(const ctr_afm_fwd_args* a, ctr_stream_t stream);

typedef struct ctr_afm_bwd_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int A; int64_t V;
  const float* emb; const float* W1; const float* b1; const float* w2; const float* b2;
  float drop_p; uint64_t seed; const float* attn; const float* dpooled; int64_t ldg;
  float* dslot; float* dW1; float* db1; float* dw2; float* db2;
  void* ws; int64_t ws_bytes; int32_t* err_flag;
} ctr_afm_bwd_args;
int ctr_op_afm_bwd(const ctr_afm_bwd_args* a, ctr_stream_t stream);

/* ctr_afm_head with its arguments in a struct (the flat entry point's contract). */
typedef struct ctr_afm_head_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* lin; const float* bias; const float* pooled; int64_t ldp;
  const float* fc_w; const float* fc_b; const float* labels; float mean_div;
  float* z; float* p; float* loss_elem; float* gz; float* dpooled; int64_t ldg;
  int32_t* err_flag;
} ctr_afm_head_args;
int ctr_op_afm_head(const ctr_afm_head_args* a, ctr_stream_t stream);

/* Wide&Deep — ctr_wd_forward / ctr_wd_embedding_grad / ctr_wd_embedding_grad_adam with their
 * arguments in a struct (the flat entry points' contract; ws sized by
 * ctr_segment_workspace_bytes). */
typedef struct ctr_wd_fwd_args {
  const void* idx; int idx_type; int64_t B; int F; int K; int64_t V;
  const float* emb; const float* lin; const float* bias;
  float* flat; int64_t ldf; const ctr_planes* x_planes; float* z_lin; int32_t* err_flag;
} ctr_wd_fwd_args;
int ctr_op_wd_fwd(const ctr_wd_fwd_args* a, ctr_stream_t stream);

typedef struct ctr_wd_embedding_grad_args {
  const ctr_sparse_plan* plan; int F; int K; const float* gz; const float* dx;
  float* grad_rows; float* grad_lin; int32_t* rowmap; void* ws; int64_t ws_bytes;
} ctr_wd_embedding_grad_args;
int ctr_op_wd_embedding_grad(const ctr_wd_embedding_grad_args* a, ctr_stream_t stream);

typedef struct ctr_wd_embedding_grad_adam_args {
  const ctr_sparse_plan* plan; int F; int K; const float* gz; const float* dx;
  const ctr_deferred_table* table; const int32_t* step_ptr; const float* step_table;
  double beta1; double beta2; double eps; double weight_decay;
  float* grad_rows; float* grad_lin; int keep_sums; void* ws; int64_t ws_bytes;
} ctr_wd_embedding_grad_adam_args;
int ctr_op_wd_embedding_grad_adam(const ctr_wd_embedding_grad_adam_args* a, ctr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CTR_HIP_H */
