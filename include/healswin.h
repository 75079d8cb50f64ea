/*
 * healswin.h -- C ABI of the MI355X-native HEAL-SWIN hot path (libhealswin.so).
 *
 * The reference (JanEGerken/HEAL-SWIN) is pure Python/PyTorch and has no FFI of its own; these are the
 * entry points a maintainer would bind (ctypes) to replace the stock-op call
 * sites of heal_swin/models_torch/{hp_windowing,hp_shifting,swin_hp_transformer}.py.  Each entry
 * point cites the reference interface it replaces as `file:line` relative to /root/reference/heal_swin/.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  Device pointers are marked [dev], host [host].
 *   - every function returns an hs_status (0 = ok); nothing throws across the ABI.
 *   - kernels never allocate or free; all buffers (outputs, workspaces) are owned by the caller.
 *   - device functions are stream-ordered on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and re-entrant (activation-checkpoint recompute calls them twice).
 *   - activations are row-major [B, N, C] ("token rows"), dtype HS_F32 or HS_BF16; statistics,
 *     softmax, bias and all accumulations are fp32 in both modes.
 *   - "natural order" = the reference's nested HEALPix pixel order; "shifted order" = after
 *     shifter.shift().  Window w of an image covers shifted positions [w*Ws, (w+1)*Ws).
 *
 * Pointer alignment
 *   The kernels move operands in 16-byte units (float4 / 8 x bf16 loads and stores, 16-byte-per-lane buffer loads into LDS), and
 *   a load whose address is not a multiple of its width does not read what the pointer arithmetic says.  Every [dev] pointer of
 *   hs_gemm_nt, hs_mlp_fused_*, hs_window_attn_module_*, hs_layernorm_* / hs_add_layernorm_*, hs_ln_head_*,
 *   hs_expand_ln_head_* (labels, targets, class weights and predictions excepted: single elements), hs_patch_merge_*,
 *   hs_patch_expand_*, hs_linear_wgrad* (members of a group and the destinations of sums queued for hs_reduce_flush included),
 *   hs_gelu_* and hs_split_bf16x3 (the bf16 output of hs_gelu_split3 and hs_split_bf16x3: 8 bytes), hs_residual_drop,
 *   hs_adam_step / hs_adam_step_guarded / hs_adam_step_groups / hs_adam_step_groups_guarded (their bf16 copy and the run table of
 *   the grouped forms: 8 bytes), hs_grad_stats and hs_grad_scale must therefore be 16-byte
 *   aligned: activations, weights, biases, gamma / beta, workspaces and gradient destinations alike.  They
 *   check it before anything is launched and return HS_ERR_MISALIGNED; the entry points that chain others check every pointer first.
 *   Entry points that address single elements take any naturally aligned pointer: hs_rel_bias_*, hs_cos_head_scale_*,
 *   hs_transpose_many_16 (whose job table lives on the device and cannot be checked), and those that choose between a vector
 *   and a scalar path from the pointer (hs_gather_rows, the flat / depth data paths, the evaluation kernels).
 *   The Python layer meets the requirement by construction.  On a GPU parallel.GradBucketAllReduce gives every parameter a slot
 *   of a multiple of 8 fp32 elements, so each gradient view -- and each parameter, moment and bf16 copy that optim.FlatAdam lays
 *   out at the same element offsets -- starts on a 32-byte (fp32) or 16-byte (bf16) boundary.  The ops take an aligned copy of
 *   any other parameter-like INPUT that is not (and of LayerNorm / GELU activations); a gradient sink that hands out a misaligned
 *   DESTINATION for a vector deposit is an error (RuntimeError), not worked around.
 */
#ifndef HEALSWIN_H
#define HEALSWIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    HS_OK = 0,
    HS_ERR_INVALID_ARG = 1,   /* reference: bare `assert` at construction / call time */
    HS_ERR_UNSUPPORTED = 2,   /* shape/dtype outside what the kernels implement */
    HS_ERR_HIP = 3,           /* a HIP runtime call failed (no device, launch failure); see hs_last_error */
    HS_ERR_NOT_PERMUTATION = 4, /* reference: _validate_shift_result, models_torch/hp_shifting.py:96-99,385-388 */
    HS_ERR_MISALIGNED = 5      /* a device pointer misses the alignment stated under "Pointer alignment" above; nothing was launched */
} hs_status;

typedef enum { HS_F32 = 0, HS_BF16 = 1 } hs_dtype;

/* flags of hs_window_attn_* */
#define HS_ATTN_COSINE 1u      /* cosine attention: L2-normalise q,k (eps 1e-12), per-head scale */
#define HS_ATTN_FORCE_VALU 2u  /* run the generic fp32-VALU kernels even where an MFMA kernel exists (cross-checks, A/B) */
#define HS_ATTN_RESIDUAL 4u    /* hs_window_attn_module_fwd: out = x + module(x) (the block's residual add, :316) */
#define HS_ATTN_OVERWRITE_GRADS 8u /* hs_window_attn_bwd, bf16 MFMA path (window 64, head_dim 32): dbias / dhead_scale are WRITTEN instead of
                                    added into (no zero fill needed); on the fp32 and VALU paths, which accumulate, the entry point
                                    zeroes both first, so the flag means the same on every path */

const char* hs_version(void);
/* human-readable message of the last failing call on this thread ("" if none) */
const char* hs_last_error(void);
const char* hs_status_string(int status);
/* number of visible HIP devices (0 on a CPU-only host); never fails */
int hs_device_count(void);

/* `count` 2-D transposes of 16-bit matrices in one launch.  jobs [dev]: `count` records {const void* src [rows, cols] row-major;
 * void* dst [cols, rows] row-major; int64 rows; int64 cols} (32 bytes each).  The per-step [in, out] copies of the Linear weights
 * (B operand of the input-gradient products of hs_gemm_nt; autograd of nn.Linear, models_torch/swin_hp_transformer.py:33-35). */
int hs_transpose_many_16(const void* jobs, int count, int blocks_per_job, void* stream);

/* Compute units that the persistent / one-resident-round launches of this library leave FREE (a multiple of 8 in [0, 128]: the same
 * number on each of the 8 XCDs; default 0, or the environment variable HS_RESERVED_CUS).  Data-parallel training (the reference's
 * Lightning DDP, train.py:182-189) runs RCCL's all-reduce kernels on their own stream DURING the backward; a kernel whose grid
 * is sized to fill every CU for its whole duration either delays them to its end or, if they were resident first, runs its
 * last workgroups as a second round.  heal_swin_amd.parallel.GradBucketAllReduce sets this when world_size > 1.
 * Affects hs_linear_wgrad (+ _workspace), hs_gemm_nt, hs_window_attn_* (+ _workspace), hs_window_attn_module_fwd(_train). */
int hs_set_reserved_cus(int n);
int hs_get_reserved_cus(void);
/* HIP-graph replay with dropout (graphs.GraphedTrainStep; replaces nothing in the reference -- its trainer draws torch's Philox
 * stream per call, `nn.Dropout` at models_torch/swin_hp_transformer.py:36, :122, :126).  Every stochastic entry point takes its seed by
 * value, so a captured launch would repeat its mask on every replay.  hs_set_seed_epoch(counter) registers a [dev] uint64 counter for
 * this process (NULL: off, the default): every mask generator then adds counter * odd constant to its seed at kernel start, and the owner
 * of the graph advances the counter once per replayed step (forward and backward of a step read the same value). */
int hs_set_seed_epoch(const void* counter);
const void* hs_get_seed_epoch(void);
/* Diagnostic: `n_workgroups` workgroups of `threads` threads and `lds_bytes` of LDS each that stay resident for `microseconds`
 * on `stream` -- a stand-in for a communication library's long-lived ring kernels (tools/cu_contention.py). */
int hs_debug_occupy_cus(int n_workgroups, int threads, int lds_bytes, double microseconds, void* stream);
/* Diagnostic (tests): one wavefront loads dword i at vector offset 4 i + scalar offset `soffset` through a raw buffer descriptor
 * over `bytes` bytes of src -- into registers (out128[0..63]) and by LDS-DMA (out128[64..127]).  Pins the hardware rule the
 * role-separated operand DMA of hs_gemm_nt relies on: the scalar offset takes part in the range check (out-of-range dwords
 * read 0), so edge tiles never fetch memory behind an operand. */
int hs_debug_buffer_soffset_probe(const void* src, int bytes, int soffset, void* out128, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Host-side HEALPix index tables, built once per model on the host (plain C++, no GPU needed).
 * ---------------------------------------------------------------------------------------------- */

/* healpy.pixelfunc.nest2ring / ring2nest as called at models_torch/hp_shifting.py:333 / :329.
 * nside must be a power of two; indices in [0, 12*nside^2).  in/out [host], n entries. */
int hs_nest2ring(int nside, const int64_t* in, int64_t* out, int64_t n);
int hs_ring2nest(int nside, const int64_t* in, int64_t* out, int64_t n);

/* get_nest_win_idcs, models_torch/hp_windowing.py:43-62.  out [host] int64[side*side], row-major. */
int hs_nest_win_idcs(int window_size, int64_t* out);

/* relative_position_index of WindowAttention.__init__, models_torch/swin_hp_transformer.py:98-114.
 * out [host] int64[Ws*Ws]. */
int hs_rel_pos_index(int window_size, int64_t* out);

/* Shifters.  All three fill
 *   idx    int32[N]  shift(x)[:, j]      = x[:, idx[j]]     (.shift)
 *   inv    int32[N]  shift_back(y)[:, i] = y[:, inv[i]]     (.shift_back), inv = idx^-1
 *   labels uint8[N]  region label of shifted position j; attention inside a window is masked with
 *                    -100 where labels differ (get_attn_mask_from_mask, models_torch/hp_shifting.py:10-28)
 * any of the three output pointers may be NULL.  N = n_pix (roll) or base_pix*nside^2 (grid, ring). */

/* NestRollShift, models_torch/hp_shifting.py:42-73 (valid for any base_pix). */
int hs_build_nest_roll_shift(int64_t n_pix, int window_size, int shift_size,
                             int32_t* idx, int32_t* inv, uint8_t* labels);
/* NestGridShift, models_torch/hp_shifting.py:76-306 (base_pix must be 8, as the reference asserts :78). */
int hs_build_nest_grid_shift(int nside, int base_pix, int window_size,
                             int32_t* idx, int32_t* inv, uint8_t* labels);
/* RingShift, models_torch/hp_shifting.py:309-404 (only valid for base_pix == 8, like the reference). */
int hs_build_ring_shift(int nside, int base_pix, int window_size, int shift_size,
                        int32_t* idx, int32_t* inv, uint8_t* labels);

/* get_attn_mask_from_mask, models_torch/hp_shifting.py:10-28: out [host] float[nW*Ws*Ws] in {0,-100}.
 * Only needed to emit the reference's `attn_mask` state-dict buffer; the kernels read `labels`. */
int hs_attn_mask_from_labels(const uint8_t* labels, int64_t n, int window_size, float* out);

/* ------------------------------------------------------------------------------------------------
 * Relative-position bias: table[rel_idx] gather and its gradient.
 * Replaces models_torch/swin_hp_transformer.py:152-159 (relative_position_bias_table[index].permute(2,0,1)).
 * ---------------------------------------------------------------------------------------------- */
/* bias[h, i, j] = table[rel_idx[i, j], h].  table [dev] f32[T, nH]; rel_idx [dev] int32[Ws*Ws];
 * bias [dev] f32[nH, Ws, Ws]. */
int hs_rel_bias_gather(const float* table, const int32_t* rel_idx, float* bias,
                       int table_rows, int num_heads, int window_size, void* stream);
/* dtable[t, h] = sum over (i,j) with rel_idx[i,j] == t of dbias[h, i, j]   (dtable is overwritten). */
int hs_rel_bias_scatter_grad(const float* dbias, const int32_t* rel_idx, float* dtable,
                             int table_rows, int num_heads, int window_size, void* stream);
/* The same with the index pre-grouped by table row: order [dev] int32[Ws*Ws] = stable argsort of rel_idx, offsets [dev]
 * int32[T + 1] = start of each row's run in `order`.  One thread per (t, h), entries added in ascending (i, j) order. */
int hs_rel_bias_scatter_grad_sorted(const float* dbias, const int32_t* order, const int32_t* offsets, float* dtable,
                                    int table_rows, int num_heads, int window_size, void* stream);
/* ... ADDED to dtable (an fp32 gradient buffer that already holds other contributions). */
int hs_rel_bias_scatter_grad_sorted_add(const float* dbias, const int32_t* order, const int32_t* offsets, float* dtable,
                                        int table_rows, int num_heads, int window_size, void* stream);
/* Cosine attention's per-head score scale, models_torch/swin_hp_transformer.py:144-147:
 *   scale[h] = exp(min(logit_scale[h], ln 100));   d logit_scale[h] = d scale[h] * scale[h] * [logit_scale[h] <= ln 100]
 * (overwritten, or added to when accumulate != 0).  All [dev] f32[num_heads]. */
int hs_cos_head_scale_fwd(const float* logit_scale, float* scale, int num_heads, void* stream);
int hs_cos_head_scale_bwd(const float* logit_scale, const float* dscale, float* dlogit_scale, int num_heads, int accumulate, void* stream);
/* The same three operations for ALL attention blocks of a model in one launch each (`count` jobs; host arrays of device pointers and
 * per-job head counts; every job shares rel_idx / order / offsets, i.e. the window size):
 *   hs_rel_bias_gather_many: bias of job j = bias_base + (heads[0] + ... + heads[j-1]) * Ws*Ws, f32[heads[j], Ws, Ws];
 *   hs_rel_bias_scatter_grad_sorted_many: dtables[j] f32[T, heads[j]] overwritten, or added to where accumulate[j] != 0;
 *   hs_cos_head_scale_many: dscale == NULL: out[j][h] = exp(min(logit_scale[j][h], ln 100)); else out[j][h] (+)= the gradient above
 *   (heads[j] <= 64).
 * More than 48 jobs run as several launches; every job is checked first, so HS_ERR_INVALID_ARG means that nothing was launched. */
int hs_rel_bias_gather_many(const void* const* tables, const int* heads, int count, const int32_t* rel_idx, float* bias_base,
                            int table_rows, int window_size, void* stream);
int hs_rel_bias_scatter_grad_sorted_many(const void* const* dbias, void* const* dtables, const int* heads, const int* accumulate, int count,
                                         const int32_t* order, const int32_t* offsets, int table_rows, int window_size, void* stream);
int hs_cos_head_scale_many(const void* const* logit_scale, const void* const* dscale, void* const* out, const int* heads, const int* accumulate,
                           int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused  shift -> window_partition -> attention core -> window_reverse -> shift_back.
 *
 * Replaces, in one kernel, models_torch/swin_hp_transformer.py:319 (shifter.shift), :322
 * (window_partition, hp_windowing.py:6-21), :136-171 of WindowAttention.forward (q/k/v split, cosine
 * or scaled QK^T, + relative position bias, + shift mask, softmax, attn @ v, head merge), :327
 * (window_reverse, hp_windowing.py:24-40) and :330 (shifter.shift_back).  Row permutations commute
 * with the row-wise qkv / proj Linear layers, so the kernel gathers rows of the *unshifted* qkv
 * tensor through `idx` and scatters its output rows back through the same `idx`.
 *
 *   qkv    [dev] dtype[B, N, 3C]  output of the qkv Linear in natural order, columns [q|k|v][head][hd]
 *   out    [dev] dtype[B, N, C]   attention output in natural order, columns [head][hd] (input of proj)
 *   lse    [dev] f32[B, nH, N]    log-sum-exp of every score row, indexed by SHIFTED position; saved
 *                                 for the backward pass (may be NULL for inference)
 *   bias   [dev] f32[nH, Ws, Ws]  or NULL (rel_pos_bias is None)
 *   head_scale [dev] f32[nH]      cosine: exp(min(logit_scale, ln 100)) (:144-147); else qk scale (:81,:149)
 *   idx    [dev] int32[N] gather table of the shifter, or NULL: then shifted position j reads token
 *                         (j + roll) mod N   (roll = 0: NoShift; roll = shift_size: NestRollShift)
 *   labels [dev] uint8[N] region labels in shifted order, or NULL (no mask; unshifted blocks)
 *   flags  HS_ATTN_COSINE and/or HS_ATTN_FORCE_VALU, or 0
 *   attn_drop, seed  attention dropout of :169 (self.attn_drop on the probabilities): each probability is zeroed with
 *                    probability attn_drop, survivors scaled by 1/(1-attn_drop); the mask is a pure function of
 *                    (seed, image, head, query, key), so hs_window_attn_bwd called with the same seed reproduces it.
 *                    attn_drop = 0 (eval mode / p = 0) disables it.
 * Supported: Ws any power of two in [4, 256], Ws <= N, N % Ws == 0, head_dim <= 128 (any value; padded to a power of two in
 * registers).  (Ws = 64, head_dim = 32 takes the MFMA paths; everything else the fp32-VALU path, whose K / V rows of a
 * workgroup must fit the LDS: the forward serves every pair but (256, head_dim > 64), the backward head_dim <= 128 up to
 * Ws 64, <= 64 at Ws 128 and <= 32 at Ws 256.  Anything else returns HS_ERR_UNSUPPORTED before anything is launched or written.)
 */
int hs_window_attn_fwd(const void* qkv, void* out, float* lse,
                       const float* bias, const float* head_scale,
                       const int32_t* idx, int64_t roll, const uint8_t* labels,
                       int batch, int64_t n_tokens, int channels, int num_heads, int window_size,
                       unsigned flags, float attn_drop, uint64_t seed, int dtype, void* stream);

/* Backward of the above.
 *   dout   [dev] dtype[B, N, C]   gradient w.r.t. `out`
 *   dqkv   [dev] dtype[B, N, 3C]  gradient w.r.t. `qkv` (every row is written exactly once)
 *   dbias  [dev] f32[nH, Ws, Ws]  ACCUMULATED into (caller zeroes it), or NULL when bias is NULL
 *   dhead_scale [dev] f32[nH]     ACCUMULATED into (caller zeroes it); only written for HS_ATTN_COSINE
 *                                 (the scaled variant's scale is a constant), may be NULL otherwise
 *   workspace [dev] f32[hs_window_attn_bwd_workspace(...)]  per-workgroup partial bias/scale gradients of the
 *                                 MFMA path (reduced deterministically, no atomics); may be NULL when the query
 *                                 returns 0 (fp32-VALU path)
 */
int64_t hs_window_attn_bwd_workspace(int batch, int64_t n_tokens, int channels, int num_heads, int window_size, int dtype);
int hs_window_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                       void* dqkv, float* dbias, float* dhead_scale, float* workspace,
                       const float* bias, const float* head_scale,
                       const int32_t* idx, int64_t roll, const uint8_t* labels,
                       int batch, int64_t n_tokens, int channels, int num_heads, int window_size,
                       unsigned flags, float attn_drop, uint64_t seed, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Standalone shift along the nested pixel axis: out[b, j, :] = x[b, idx[j], :]  (idx NULL: roll,
 * out[b, j, :] = x[b, (j + roll) mod N, :]).  Replaces shifter.shift / shift_back when called on their
 * own: models_torch/hp_shifting.py:69-73 (torch.roll), :302-306 and :400-404 (x[:, idcs].contiguous()).
 * Pass `inv` as idx for shift_back.  Not on the model's path (the permutation is fused into
 * hs_window_attn_*); used by the shifter API and by the gather/scatter bandwidth measurement.
 *   x, out [dev] distinct buffers of batch * n_tokens rows of row_bytes bytes each.
 * ---------------------------------------------------------------------------------------------- */
int hs_gather_rows(const void* x, void* out, const int32_t* idx, int64_t roll,
                   int batch, int64_t n_tokens, int64_t row_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row LayerNorm over contiguous rows (eps = 1e-5, affine), optionally fused with a residual add.
 * This is the normalisation half of PatchMerging (LayerNorm over the 4C row formed by 4 sibling
 * pixels, models_torch/swin_hp_transformer.py:385-392: the slicing + cat is a free view in nested
 * order), of PatchExpand / FinalPatchExpand_X4 (LayerNorm over each C/p child row after the
 * 'b n (p c) -> b (n p) c' view, :427-428, :449-450) and of the block norms (:316, :334-338, :945, :781).
 *
 *   y = LN(x) * gamma + beta               (residual == NULL)
 *   y = residual + LN(x) * gamma + beta    (v2 norm placement, :334-335)
 *   x, y, residual [dev] dtype[rows, width]; gamma, beta [dev] f32[width];
 *   mean, rstd [dev] f32[rows] saved for backward (may be NULL for inference).
 */
int hs_layernorm_fwd(const void* x, const void* residual, const float* gamma, const float* beta,
                     void* y, float* mean, float* rstd,
                     int64_t rows, int width, int dtype, void* stream);
/* dx [dev] dtype[rows, width]; dgamma, dbeta [dev] f32[width]: sum over all rows, OVERWRITTEN, or ADDED to
 * the existing contents when accumulate != 0 (a parameter's fp32 .grad buffer).
 * The residual branch's gradient is dy itself (identity) and is not produced here.
 * workspace [dev] f32[hs_layernorm_bwd_workspace(rows, width)] */
int64_t hs_layernorm_bwd_workspace(int64_t rows, int width);
int hs_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                     void* dx, float* dgamma, float* dbeta, float* workspace, int accumulate,
                     int64_t rows, int width, int dtype, void* stream);

/* Fused residual add + LayerNorm (v1 norm placement, models_torch/swin_hp_transformer.py:337-338 and :316 of the
 * following block):   sum = a + b (stored in the activation dtype),  y = LN(sum) * gamma + beta.
 * Backward: dx = LN_bwd(dy) + dsum, which is the gradient of BOTH a and b (dsum may be NULL: no other consumer of sum);
 * `sum` is the tensor saved by the forward; workspace as for hs_layernorm_bwd. */
int hs_add_layernorm_fwd(const void* a, const void* b, const float* gamma, const float* beta,
                         void* sum_out, void* y, float* mean, float* rstd,
                         int64_t rows, int width, int dtype, void* stream);
int hs_add_layernorm_bwd(const void* dy, const void* dsum, const void* sum, const float* gamma,
                         const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta, float* workspace,
                         int accumulate, int64_t rows, int width, int dtype, void* stream);

/* Train-mode variants with the block's stochastic regularisers fused in (models_torch/swin_hp_transformer.py:173 proj_drop,
 * :43 Mlp output dropout, :334-338 DropPath): drop() is a counter-based dropout mask (drop_p, seed; regenerated by the
 * backward called with the same seed), rs = row_scale[row / rows_per_sample] the per-sample DropPath factor
 * (0 or 1/keep; row_scale [dev] f32[rows / rows_per_sample], may be NULL = 1).
 *   hs_layernorm_drop_*      (v2 placement):  y = [residual +] rs * LN(drop(x));        dx = mask * LN_bwd(rs * dy)
 *   hs_add_layernorm_drop_*  (v1 placement):  sum = a + rs * drop(b),  y = LN(sum);     da = g, db = rs * mask * g
 *                                             with g = LN_bwd(dy) + dsum */
int hs_layernorm_drop_fwd(const void* x, const void* residual, const float* gamma, const float* beta, void* y,
                          float* mean, float* rstd, const float* row_scale, int64_t rows_per_sample, float drop_p,
                          uint64_t seed, int64_t rows, int width, int dtype, void* stream);
int hs_layernorm_drop_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                          void* dx, float* dgamma, float* dbeta, float* workspace, int accumulate, const float* row_scale,
                          int64_t rows_per_sample, float drop_p, uint64_t seed, int64_t rows, int width, int dtype,
                          void* stream);
int hs_add_layernorm_drop_fwd(const void* a, const void* b, const float* gamma, const float* beta, void* sum_out, void* y,
                              float* mean, float* rstd, const float* row_scale, int64_t rows_per_sample, float drop_p,
                              uint64_t seed, int64_t rows, int width, int dtype, void* stream);
/* General forward with every optional operand, incl. the COMPENSATED RESIDUAL STREAM (replaces the reference's two plain adds per
 * block, swin_hp_transformer.py:316 / :338 (v1) and :334-335 (v2), whose results it keeps to 16 instead of 8 mantissa bits in bf16):
 * exactly one of `residual` (v2: y = residual + rs LN(drop(x))) and `add_in` (v1: sum_out = x + rs drop(add_in), y = LN(sum_out)).
 * lo_in (optional) is the rounding remainder of the stream operand (x for v1, residual for v2) left by the previous call, lo_out
 * (optional) receives the remainder of the new stream (sum_out for v1, y for v2; for a plain LayerNorm -- neither residual nor add_in
 * -- the rounding remainder of y, for a consumer that takes its operand as hi + lo: hs_expand_ln_head_fwd): stream = hi + lo with hi
 * the plain activation tensor every other kernel reads.  Backward: the plain hs_*layernorm*_bwd entry points on the hi tensors. */
int hs_layernorm_fwd_ex(const void* x, const void* residual, const void* add_in, const void* lo_in, const float* gamma,
                        const float* beta, void* y, void* sum_out, void* lo_out, float* mean, float* rstd,
                        const float* row_scale, int64_t rows_per_sample, float drop_p, uint64_t seed, int64_t rows, int width,
                        int dtype, void* stream);
int hs_add_layernorm_drop_bwd(const void* dy, const void* dsum, const void* sum, const float* gamma, const float* mean,
                              const float* rstd, void* da, void* db, float* dgamma, float* dbeta, float* workspace, int accumulate,
                              const float* row_scale, int64_t rows_per_sample, float drop_p, uint64_t seed,
                              int64_t rows, int width, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * y = dropout(GELU(x)) (exact erf GELU) and its backward dx = dy * mask/(1-p) * GELU'(x): the activation and the
 * dropout behind it in Mlp.forward (models_torch/swin_hp_transformer.py:39-41) in one pass.  drop_p = 0 (eval) is plain
 * GELU.  The mask is a pure function of (seed, element index): pass the forward's seed to the backward.
 * x, y, dy, dx [dev] dtype[n], 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int hs_gelu_fwd(const void* x, void* y, int64_t n, float drop_p, uint64_t seed, int dtype, void* stream);
int hs_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, float drop_p, uint64_t seed, int dtype, void* stream);

/* out = x + rs * drop(t): a residual branch added in its standalone form (end of a stage; dropout on the branch output
 * models_torch/swin_hp_transformer.py:43, :173 and DropPath :334-338 in one pass).  rs = row_scale[i / elems_per_sample]
 * (row_scale [dev] f32[n / elems_per_sample], NULL = 1); x == NULL gives out = rs * drop(t), which is also the backward:
 * dt = hs_residual_drop(NULL, dy, ...) with the forward's seed (dx = dy). */
int hs_residual_drop(const void* x, const void* t, void* out, const float* row_scale, int64_t elems_per_sample, int64_t n,
                     float drop_p, uint64_t seed, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Class-weighted cross-entropy of the segmentation caller (reference: nn.CrossEntropyLoss(weight)(logits[B,K,Npix],
 * labels.long()[B,Npix]), models_lightning/segmentation/model_lightning_swin_hp.py:39-45, :104-111):
 *     loss = sum_i w[y_i] (logsumexp_c z_i[c] - z_i[y_i]) / sum_i w[y_i]
 * logits [dev] dtype, element (b, c, pixel) at b*stride_b + c*stride_k + pixel*stride_p (so the model's native
 * [B, Npix, K] output viewed as [B, K, Npix] needs no copy); labels [dev] uint8 / int32 / int64 (label_bytes 1/4/8)
 * [batch, npix] contiguous; class_weights [dev] f32[n_classes] or NULL; pixels labelled ignore_index (or out of range)
 * are skipped.  n_classes <= 64.
 *   hs_seg_ce_fwd: partials [dev] f32[hs_seg_ce_partials(batch, npix)][2] = per-workgroup (numerator, denominator);
 *                  the caller sums them (fixed order) and divides.
 *   hs_seg_ce_bwd: dlogits (own strides) = scale[0] * w[y] * (softmax(z) - onehot(y)), scale [dev] f32[1] =
 *                  upstream gradient / denominator (a device scalar: no host synchronisation).
 * ---------------------------------------------------------------------------------------------- */
int64_t hs_seg_ce_partials(int64_t batch, int64_t npix);
int hs_seg_ce_fwd(const void* logits, const void* labels, const float* class_weights, float* partials,
                  int64_t batch, int64_t npix, int n_classes, int64_t stride_b, int64_t stride_k, int64_t stride_p,
                  int label_bytes, int64_t ignore_index, int dtype, void* stream);
int hs_seg_ce_bwd(const void* logits, const void* labels, const float* class_weights, const float* scale, void* dlogits,
                  int64_t batch, int64_t npix, int n_classes, int64_t stride_b, int64_t stride_k, int64_t stride_p,
                  int64_t dstride_b, int64_t dstride_k, int64_t dstride_p, int label_bytes, int64_t ignore_index,
                  int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth-regression losses of the depth caller (reference: heal_swin/training/loss_depth_regression.py, as
 * heal_swin_amd/losses.py restates it), d = pred[:, 0] - target over the pixels whose target is not infinite (NaN targets are kept):
 *     HS_DEPTH_L1 mean |d|,  HS_DEPTH_L2 mean d^2 / 2,  HS_DEPTH_HUBER SmoothL1(beta = huber_delta) (channels == 1 only),
 *     HS_DEPTH_LOGVAR mean pred[:, 1] / 2 + d^2 exp(-pred[:, 1]) / 2 (channels >= 2).
 * pred [dev] dtype HS_F32 / HS_BF16, element (b, c, pixel) at b*stride_b + c*stride_c + pixel*stride_p (the model's padded
 * [B, Npix, 16] rows seen as [B, f_out, Npix] need no copy), channels <= 16; target [dev] f32[batch, npix] contiguous.
 *   hs_depth_loss_fwd: partials [dev] f32[hs_depth_loss_partials(batch, npix)][2] = per-workgroup (sum, kept count); the caller
 *                      sums them (fixed order) and divides (no kept pixel: 0 / 0 = NaN, as the reference's mean of nothing).
 *   hs_depth_loss_bwd: dpred (own strides, every channel written) = scale[0] * dterm / dpred at kept pixels, exactly 0 elsewhere
 *                      and in the channels the kind does not read; scale [dev] f32[1] = upstream gradient / kept count.
 * ---------------------------------------------------------------------------------------------- */
#define HS_DEPTH_L1 0
#define HS_DEPTH_L2 1
#define HS_DEPTH_HUBER 2
#define HS_DEPTH_LOGVAR 3
int64_t hs_depth_loss_partials(int64_t batch, int64_t npix);
int hs_depth_loss_fwd(const void* pred, const float* target, float* partials, int64_t batch, int64_t npix, int channels,
                      int64_t stride_b, int64_t stride_c, int64_t stride_p, int kind, float huber_delta, int dtype, void* stream);
int hs_depth_loss_bwd(const void* pred, const float* target, const float* scale, void* dpred, int64_t batch, int64_t npix, int channels,
                      int64_t stride_b, int64_t stride_c, int64_t stride_p, int64_t dstride_b, int64_t dstride_c, int64_t dstride_p,
                      int kind, float huber_delta, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight / bias gradient of the path's Linear layers (autograd of nn.Linear at
 * models_torch/swin_hp_transformer.py:33,:35 (Mlp), :116,:118 (qkv, proj), :375 (PatchMerging.reduction), :415-416
 * (PatchExpand.expand), :438, :717 (concat_back_dim)):
 *     dw[n, k] = sum_m dy[m, n] * x[m, k]        dbias[n] = sum_m dy[m, n]
 *   dy [dev] dtype[rows, n_out], x [dev] dtype[rows, k_in] (row-major token rows); dw [dev] f32[n_out, k_in] and
 *   dbias [dev] f32[n_out] (may be NULL) are overwritten (accumulate == 0) or added to (accumulate != 0: the
 *   caller's .grad buffers); workspace [dev] f32[hs_linear_wgrad_workspace(...)].
 * dtype HS_BF16: dy, x bf16; k_in a multiple of 8, n_out a multiple of 4 (of 8 when a token slice exceeds 2 GiB).
 * dtype HS_F32: dy, x f32 (v_mfma_f32_32x32x2_f32); n_out and k_in multiples of 4.
 * Split over the token axis, deterministic.
 * ---------------------------------------------------------------------------------------------- */
int64_t hs_linear_wgrad_workspace(int64_t rows, int n_out, int k_in);
int hs_linear_wgrad(const void* dy, const void* x, float* dw, float* dbias, float* workspace,
                    int64_t rows, int n_out, int k_in, int accumulate, int dtype, void* stream);
/* dw[n, k] = sum_m dy[m, n] * gelu(h[m, k]): the weight gradient of a Linear whose input is gelu(h), taken from the saved
 * pre-activation h (fc2 of reference Mlp.forward :38-44) -- the fused Mlp block then keeps h only.  Exact-erf GELU as everywhere
 * (csrc/hs_gelu.h), applied to the MFMA operand fragments; bf16 and the shapes of hs_linear_wgrad_gelu_supported (the 128 x 128
 * tile: C <= 128-class layers, whose launches are HBM-bound and have the VALU slots). */
int hs_linear_wgrad_gelu_supported(int64_t rows, int n_out, int k_in, int dtype);
int hs_linear_wgrad_gelu(const void* dy, const void* h, float* dw, float* dbias, float* workspace, int64_t rows, int n_out, int k_in,
                         int accumulate, int dtype, void* stream);
/* Several weight gradients over the SAME token rows in one launch (the Linear layers of one block half: fc2 + fc1, proj + qkv).
 * A launch is one resident round of workgroups whatever the layer is, so the slice count follows from the number of output tiles;
 * with the tiles of 2-4 layers in one launch each layer needs that many fewer token slices, i.e. fewer partial tiles to write and to
 * sum.  A problem is what the single entry points take: dy [rows, n_out], x [rows, k_in] (gelu_x != 0: x is the pre-activation
 * and gelu(x) the operand, as hs_linear_wgrad_gelu), dw, dbias (may be NULL), accumulate (bit 0 | HS_ACC_DEFER), per problem.
 * Problems share one launch when each of them alone takes the same LDS-DMA tile (hs_linear_wgrad_group_variant: equal and non-zero;
 * 1 = 256 x 256, 2 = 256 x 128, 3 = 128 x 128; bf16 only); otherwise the call launches them one by one, as the single entry points
 * would.  Results equal those of the single entry points up to the summation order over the token slices (deterministic either way).
 * workspace [dev] f32[hs_linear_wgrad_group_workspace(...)]: every problem has its own partial records in it, so a deferring caller
 * keeps it until the flush, as with the single entry points. */
typedef struct hs_wgrad_problem {
    const void* dy;
    const void* x;
    float* dw;
    float* dbias;
    int n_out, k_in, accumulate, gelu_x;
} hs_wgrad_problem;
int hs_linear_wgrad_group_variant(int64_t rows, int n_out, int k_in, int dtype);
int64_t hs_linear_wgrad_group_workspace(const hs_wgrad_problem* problems, int count, int64_t rows, int dtype);
int hs_linear_wgrad_group(const hs_wgrad_problem* problems, int count, float* workspace, int64_t rows, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Deferred parameter-gradient reductions.  hs_linear_wgrad / hs_linear_wgrad_ld and the four LayerNorm backward entry points
 * (hs_layernorm_bwd, hs_add_layernorm_bwd, hs_layernorm_drop_bwd, hs_add_layernorm_drop_bwd) end in a small "sum the
 * per-workgroup partial records into dw / dbias (dgamma / dbeta)" launch.  With HS_ACC_DEFER or-ed into `accumulate` that sum is
 * QUEUED on the call's stream instead of launched; hs_reduce_flush(stream) folds every queued sum of that stream in ONE launch
 * (deterministic order; the queue also flushes itself when it is full).  Contract of a deferring caller: the call's `workspace`
 * stays allocated and untouched until the flush, and nobody reads the gradient buffers before it.  The sums of one flush run
 * side by side without atomics, so two PENDING sums never share a destination element: a call whose dw / dbias range overlaps
 * a pending one (a parameter used twice in a backward, the bf16x3 products of an fp32 weight gradient, micro-batches without a
 * flush in between) flushes the queue first, and so does an immediate (non-deferred) sum into such a range -- issue order is
 * stream order either way.  Destination buffers must outlive the flush: flush before freeing gradient buckets.  The reference has no
 * counterpart (autograd of nn.Linear / nn.LayerNorm, models_torch/swin_hp_transformer.py:33-35, :116-118, :256-262): this is
 * how 340 launches per HEAL-SWIN-B training step become about 10.
 * ---------------------------------------------------------------------------------------------- */
#define HS_ACC_DEFER 2 /* or-ed into `accumulate` (bit 0: add to the existing contents) */
int hs_reduce_pending(void* stream); /* queued sums of that stream */
int hs_reduce_flush(void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused Mlp block of the HBM-bound stages (C = 96 / 128, hidden = 4 C; csrc/mlp_fused.hip): replaces, in ONE launch per direction,
 *   forward   the block's second residual branch  out = x + fc2(gelu(fc1(LayerNorm(x))))
 *             (models_torch/swin_hp_transformer.py:337-338 with Mlp.forward :38-44 and norm2 :262; v1 norm placement)
 *   backward  the input-gradient half of Mlp's autograd:  dh = (dy W2) * gelu'(h),  dn = dh W1
 * hs_mlp_fused_fwd: x, out [dev] bf16[rows, C]; ln_gamma, ln_beta [dev] f32[C] (both NULL: no LayerNorm in front);
 *   w1 [dev] bf16[4C, C], b1 f32[4C] | NULL, w2 [dev] bf16[C, 4C], b2 f32[C] | NULL (nn.Linear layouts);
 *   saved for the backward, each may be NULL (not kept): n_out bf16[rows, C] = LayerNorm(x), mean_out / rstd_out f32[rows],
 *   h_out bf16[rows, 4C] = fc1 output, act_out bf16[rows, 4C] = gelu(h);  flags: HS_ATTN_RESIDUAL adds x to the result.
 * hs_mlp_fused_bwd: dy [dev] bf16[rows, C], h [dev] bf16[rows, 4C] (saved), w2_t [dev] bf16[4C, C] and w1_t [dev] bf16[C, 4C] = the
 *   TRANSPOSED weights; writes dh [dev] bf16[rows, 4C] (operand of fc1's weight gradient) and dn [dev] bf16[rows, C] = dh W1 (+ dres
 *   [dev] bf16[rows, C] when non-NULL: the residual path's gradient of the v2 placement, added in the epilogue; v1: the gradient of
 *   LayerNorm(x)).  Weight / bias / LayerNorm gradients: hs_linear_wgrad(dy, gelu(h)), hs_linear_wgrad(dh, n), hs_add_layernorm_bwd.
 * rows: a multiple of 32.  HS_ERR_UNSUPPORTED outside hs_mlp_fused_supported (the weights live in registers: C <= 128).
 * ---------------------------------------------------------------------------------------------- */
#define HS_MLP_NORM_AFTER 16u /* hs_mlp_fused_fwd flags: v2 norm placement (:334-335), out = x + LayerNorm(fc2(gelu(fc1(x)))): ln_gamma / ln_beta
                                 apply BEHIND the Mlp, n_out receives the un-normalised rows mlp(x) (the LayerNorm backward's input) and
                                 mean_out / rstd_out their statistics */
int hs_mlp_fused_supported(int channels, int hidden, int dtype);
int hs_mlp_fused_fwd(const void* x, const float* ln_gamma, const float* ln_beta, const void* w1, const float* b1, const void* w2,
                     const float* b2, void* n_out, float* mean_out, float* rstd_out, void* h_out, void* act_out, void* out, int64_t rows,
                     int channels, int hidden, unsigned flags, int dtype, void* stream);
int hs_mlp_fused_bwd(const void* dy, const void* h, const void* w2_t, const void* w1_t, const void* dres, void* dh, void* dn, int64_t rows,
                     int channels, int hidden, int dtype, void* stream);
/* Train-mode form of the v2 placement with the branch's regularisers inside the launch (flags must carry HS_MLP_NORM_AFTER):
 *   out = x + rs * LayerNorm(drop_o(fc2(drop_h(gelu(fc1(x))))))       Mlp.drop behind the activation and behind fc2 (:41, :43), DropPath (:335)
 * drop_h / drop_o are the counter-based masks of hs_gemm_nt's GELU epilogue (seed_hidden, element index in [rows, 4C]) and of
 * hs_layernorm_drop_fwd (seed_out, [rows, C]); rs = row_scale[row / rows_per_sample] (row_scale [dev] f32 or NULL; rows_per_sample a multiple
 * of 32).  m_out = fc2's output BEFORE drop_o (hs_layernorm_drop_bwd regenerates the mask), mean_out / rstd_out the statistics of the dropped
 * rows, act_out = the dropped activation (operand of fc2's weight gradient).  Backward: hs_layernorm_drop_bwd(dout, m_out, ...) -> dm, then
 * hs_mlp_fused_drop_bwd(dm, h, ..., dres = dout): dh = (dm W2) * mask_h * gelu'(h), dn = dh W1 + dres. */
int hs_mlp_fused_drop_fwd(const void* x, const float* ln_gamma, const float* ln_beta, const void* w1, const float* b1, const void* w2,
                          const float* b2, void* m_out, float* mean_out, float* rstd_out, void* h_out, void* act_out, void* out,
                          const float* row_scale, int64_t rows_per_sample, float drop_p, uint64_t seed_hidden, uint64_t seed_out,
                          int64_t rows, int channels, int hidden, unsigned flags, int dtype, void* stream);
int hs_mlp_fused_drop_bwd(const void* dy, const void* h, const void* w2_t, const void* w1_t, const void* dres, void* dh, void* dn,
                          float drop_p, uint64_t seed_hidden, int64_t rows, int channels, int hidden, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer step over flat buffers: torch.optim.Adam / AdamW (the reference's training/optimizer.py:57-66; amsgrad = False,
 * maximize = False) on n consecutive fp32 parameters p with gradients g and moments m, v, all [dev] f32[n], 16-byte aligned:
 *     g += wd p (decoupled == 0)  |  p *= 1 - lr wd (decoupled != 0: AdamW)
 *     m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   t = *step + 1 with step [dev] int64 (the steps taken so far; hs_adam_advance adds 1 after the last buffer of a step);
 *   lr_dev [dev] f32[1] overrides lr when non-NULL; p_bf16 [dev] bf16[n] (may be NULL) receives the updated parameters rounded to
 *   bf16 -- the copy the next forward's GEMMs read, written from the registers that hold the new value.
 * ---------------------------------------------------------------------------------------------- */
int hs_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                 float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, void* stream);
int hs_adam_advance(int64_t* step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same step with PARAMETER GROUPS (torch's param_groups: per-group lr, betas, eps, weight decay), still one launch per buffer.
 *   groups [HOST] hs_adam_group[n_groups], 1 <= n_groups <= HS_ADAM_MAX_GROUPS: read during the call and passed to the kernel by
 *                 value -- no copy to the device, capturable; a captured launch keeps the values it was captured with, so under
 *                 graph replay a learning rate that changes is a group's lr_dev ([dev] f32[1], overrides lr when non-NULL; groups
 *                 with and without one mix freely).
 *   runs   [dev] int32[n_runs][2] = (first element, group) of each run, 8-byte aligned: a run is a maximal stretch of consecutive
 *                 parameter slots of ONE group, the alignment gap behind a slot included.  First elements ascend from 0 and are
 *                 multiples of 8 (parallel.GradBucketAllReduce's slot rule: a float4 never straddles two runs); run r ends where
 *                 run r + 1 starts, the last one at `covered`, the element count the table was built for, which must equal n.
 *                 1 <= n_runs <= ceil(n / 8); n < 2^31.
 *   block_first [dev] int32[n_blocks], n_blocks == ceil(n / 1024): the run that holds element 1024 b.  A thread starts there and
 *                 walks forward to the run of its own element.
 *   Static per buffer: optim.group_tables builds both once.  The kernel cannot be sent outside the two tables by their contents
 *   (a run index is clamped, a group index taken modulo n_groups); what they assign wrongly is stepped with the wrong group.
 *   Each workgroup resolves the n_groups records into LDS first -- lr, and the two bias corrections of ITS betas in double -- and
 *   every element is then stepped with the arithmetic of hs_adam_step and the record of its run's group: with equal records the
 *   result is bit-identical to hs_adam_step.  The zero gaps of the buffers (p = g = m = v = 0) stay zero for every record.
 *   hs_adam_step_groups_guarded is hs_adam_step_guarded in the same way (the guard section below): ONE clip coefficient, from the
 *   norm over all groups, one clip_value, one finite flag -- a skipped step skips every group -- and one step counter, advanced by
 *   hs_adam_advance / hs_adam_advance_guarded as before.
 * HS_ERR_INVALID_ARG (nothing is launched): null pointer, n <= 0 or >= 2^31, n_groups outside 1 ... HS_ADAM_MAX_GROUPS, a group
 * with beta outside [0, 1), eps < 0, weight_decay < 0 or a NaN lr, n_runs or n_blocks that do not fit n, covered != n, clip_value
 * NaN; HS_ERR_MISALIGNED ("Pointer alignment"): p, g, m, v, guard not 16-byte aligned, p_bf16 or runs not 8-byte aligned,
 * block_first or an lr_dev not 4-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define HS_ADAM_MAX_GROUPS 32
typedef struct {
    const float* lr_dev; /* [dev] f32[1] or NULL */
    float lr;
    float beta1, beta2, eps, weight_decay;
    int32_t decoupled; /* 0: g += wd p (Adam); != 0: p *= 1 - lr wd (AdamW) */
} hs_adam_group;
int hs_adam_max_groups(void); /* HS_ADAM_MAX_GROUPS of the library that was loaded */
int hs_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const hs_adam_group* groups, int n_groups,
                        const int32_t* runs, int n_runs, const int32_t* block_first, int n_blocks, int64_t covered, const int64_t* step,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Guard rails of the flat optimizer step: gradient norms, clipping and the non-finite skip -- the reference trainer's
 * gradient_clip_val / gradient_clip_algorithm, track_grad_norm and terminate_on_nan (training/train_config.py:65-66,76,104) --
 * as ONE read-only pass over the flat gradient buckets, everything decided on the device (capturable in a HIP graph).
 *
 *   hs_grad_stats      one launch per bucket g [dev] f32[n], 16-byte aligned.  items [dev] int64[n_items][2] = (start, len) in
 *                      elements of g: a slice of ONE parameter, start a multiple of 4, 0 < len <= hs_grad_guard_piece(),
 *                      start + len <= n (an item outside g reads nothing and records NaN).  One wavefront per item; writes
 *                      partials [dev] f64[n_items][2] = (sum of squares, max |g|), every element converted to double before it
 *                      is squared, every sum in double.  A NaN element makes both records NaN.
 *   hs_grad_guard_finalize   partials = the n_items records of ALL buckets, params [dev] int32[n_params][2] = (first item, item
 *                      count) of each parameter in that numbering (a parameter outside the records reads nothing and gets NaN).
 *                      Folds the items of a parameter (one wavefront each) and the parameters into the total, in an order fixed
 *                      by the two tables alone: no atomics, nothing depends on the grid, the CU count or hs_set_reserved_cus, so
 *                      two calls on the same gradients give the same bits -- on every rank of a data-parallel run that holds
 *                      the same averaged buckets.  Writes
 *                      param_norm [dev] f32[n_params] (norm_inf == 0: the 2-norm; != 0: max |g|, exact) and *guard:
 *                          total_norm   the norm of all gradients, before clipping
 *                          clip_coef    min(1, max_norm / (total_norm + 1e-6)) in fp32, evaluated as
 *                                       torch.nn.utils.clip_grad_norm_ evaluates it (reciprocal, then product); 1 when
 *                                       max_norm < 0 (no clipping by norm)
 *                          finite       1 if the total sum of squares is finite, else 0
 *                      work [dev] f64[n_params][2]: scratch.  Two small launches.
 *   hs_adam_step_guarded     hs_adam_step on the gradient  clamp(g, -clip_value, clip_value) [clip_value > 0]  * guard->clip_coef
 *                      (weight decay of the non-decoupled form is added after that: torch's clip_grad_*_ followed by step()).
 *                      With skip_nonfinite != 0 and guard->finite == 0 the launch writes nothing.  With clip_coef == 1,
 *                      finite == 1 and clip_value <= 0 the result is bit-identical to hs_adam_step.
 *   hs_adam_step_groups_guarded   the same for hs_adam_step_groups (the section above).
 *   hs_adam_advance_guarded  adds 1 to *step, or -- skip_nonfinite != 0 and guard->finite == 0 -- 0 to *step and 1 to *skipped.
 *   hs_grad_scale      the same clamp and scale applied in place to a bucket (for callers that keep another optimizer).
 * No allocation, no synchronisation.  HS_ERR_INVALID_ARG: null pointer, n <= 0; HS_ERR_MISALIGNED: g, p, m, v, partials, work,
 * items not 16-byte aligned (p_bf16, params: 8; guard: 16).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    float total_norm;
    float clip_coef;
    int32_t finite;
    int32_t reserved;
} hs_grad_guard;
int hs_grad_guard_piece(void);
int hs_grad_stats(const float* g, int64_t n, const int64_t* items, int n_items, double* partials, void* stream);
int hs_grad_guard_finalize(const double* partials, int64_t n_items, const int32_t* params, int n_params, int norm_inf, float max_norm,
                           float* param_norm, double* work, hs_grad_guard* guard, void* stream);
int hs_adam_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                         float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, float clip_value,
                         const hs_grad_guard* guard, int skip_nonfinite, void* stream);
int hs_adam_step_groups_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const hs_adam_group* groups,
                                int n_groups, const int32_t* runs, int n_runs, const int32_t* block_first, int n_blocks, int64_t covered,
                                const int64_t* step, float clip_value, const hs_grad_guard* guard, int skip_nonfinite, void* stream);
int hs_adam_advance_guarded(int64_t* step, const hs_grad_guard* guard, int skip_nonfinite, int64_t* skipped, void* stream);
int hs_grad_scale(float* g, int64_t n, float clip_value, const hs_grad_guard* guard, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight averaging over the flat buffers: SWA -- the reference trainer's stochastic_weight_avg (training/train_config.py:112), i.e.
 * torch.optim.swa_utils.AveragedModel with its default equal average -- and EMA, the same thing at every step.  The average avg
 * [dev] f32[n] is laid out like the parameters p [dev] f32[n] of hs_adam_step (both 16-byte aligned); n_averaged [dev] int64[1]
 * counts the updates taken so far and is read ON THE DEVICE, so a captured step replays with the right weight.
 *
 *   hs_weight_avg_update    one launch per buffer, 8 B read + 4 B written per element:
 *                               *n_averaged == 0:  avg = p   (AveragedModel.update_parameters' first call; bit for bit)
 *                               otherwise:         avg = w < 0.5 ? avg + w (p - avg) : p - (p - avg)(1 - w)    (ATen's lerp, fp32)
 *                               kind 0 (SWA): w = 1.f / (float)(*n_averaged + 1);   kind 1 (EMA): w = 1.f - decay
 *                           guard may be NULL.  With guard, skip_nonfinite != 0 and guard->finite == 0 -- the optimizer step this
 *                           update follows was dropped (hs_adam_step_guarded) -- the launch writes nothing.
 *   hs_weight_avg_advance   adds 1 to *n_averaged unless the update was skipped by the same rule; after the last buffer of an update,
 *                           as hs_adam_advance.
 *   hs_weight_avg_swap      exchanges p and avg in place, 8 B read + 8 B written per element (10 with the copy).  p_bf16 [dev] bf16[n]
 *                           (may be NULL; 8-byte aligned) receives the NEW p rounded to bf16, as hs_adam_step writes it.  Bits are
 *                           moved, not computed: two swaps restore p, avg and the copy exactly.
 * No allocation, no synchronisation, capturable.  Every refusal is HS_ERR_INVALID_ARG and is decided before anything is launched: a
 * null avg, p or n_averaged, n <= 0 or >= 2^40, kind outside {0, 1}, decay outside [0, 1] (a NaN included), avg or p off a 16-byte
 * boundary, p_bf16 off an 8-byte one, n_averaged or guard off its natural alignment, p == avg in the swap.
 * ---------------------------------------------------------------------------------------------- */
int hs_weight_avg_update(float* avg, const float* p, int64_t n, int kind, float decay, const int64_t* n_averaged, const hs_grad_guard* guard,
                         int skip_nonfinite, void* stream);
int hs_weight_avg_advance(int64_t* n_averaged, const hs_grad_guard* guard, int skip_nonfinite, void* stream);
int hs_weight_avg_swap(float* p, float* avg, void* p_bf16, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused WindowAttention MODULE forward (inference form here, training form and the module backward below): the whole of WindowAttention.forward,
 * models_torch/swin_hp_transformer.py:124-174 -- qkv Linear, head split, (cosine | scaled) scores, relative-position bias,
 * shift mask, softmax, P V, head merge, proj Linear -- with the shift / window partition / reverse / shift back of
 * SwinTransformerBlock.forward (:319-330) and optionally the block's norm1 in front (:315) and residual add behind (:316):
 *     out[b, t, :] = [x[b, t, :] +] proj( attention( qkv( [LayerNorm](x) ) ) )[b, t, :]
 * in ONE launch: x is read once, out written once; qkv [B, N, 3C] and the attention output never exist in HBM
 * (SURVEY 8b's proposed entry point, 8d's fused-module roofline).
 *   x, out      [dev] bf16 [batch, n_tokens, channels], natural order; out may not alias x
 *   qkv_w       [dev] bf16 [3 * channels, channels] (nn.Linear layout, rows [q | k | v][head][32]); qkv_b [dev] f32 or NULL
 *   proj_w      [dev] bf16 [channels, channels]; proj_b [dev] f32 [channels] or NULL
 *   ln_gamma/ln_beta [dev] f32 [channels] or both NULL (eps 1e-5)
 *   bias, head_scale, idx, roll, labels: as hs_window_attn_fwd.  flags: HS_ATTN_COSINE, HS_ATTN_RESIDUAL.
 * Supported where the qkv weights fit the LDS: dtype HS_BF16, window_size 64, head_dim 32, channels 96 or 128 (stage 0 of
 * HEAL-SWIN-T / -B); everything else returns HS_ERR_UNSUPPORTED (hs_window_attn_module_supported tells beforehand) and the
 * caller composes hs_gemm_nt / hs_window_attn_fwd / hs_gemm_nt.  No dropout (inference).
 * ---------------------------------------------------------------------------------------------- */
int hs_window_attn_module_supported(int channels, int num_heads, int window_size, int dtype);
int hs_window_attn_module_fwd(const void* x, void* out, const void* qkv_w, const float* qkv_b, const void* proj_w,
                              const float* proj_b, const float* ln_gamma, const float* ln_beta, const float* bias,
                              const float* head_scale, const int32_t* idx, int64_t roll, const uint8_t* labels, int batch,
                              int64_t n_tokens, int channels, int num_heads, int window_size, unsigned flags, int dtype,
                              void* stream);

/* TRAINING form of the module forward (reference :315-316 around :124-174): the same single launch,
 *     out = [x +] proj( attention( qkv( [LayerNorm](x) ) ) )        (flags: HS_ATTN_RESIDUAL as above; v1 norm placement: LayerNorm +
 *                                                                     residual, v2 placement (:334-335): neither -- xn_out, mean_out,
 *                                                                     rstd_out NULL then, the qkv Linear's input is x itself)
 * which ALSO writes, in natural token order, everything the backward of the four reference modules reads -- so that
 * hs_add_layernorm_bwd (norm1), hs_linear_wgrad + hs_gemm_nt (qkv, proj) and hs_window_attn_bwd run on them unchanged:
 *   xn_out   [dev] bf16 [batch, n_tokens, channels]      LayerNorm(x): the qkv Linear's input
 *   mean_out, rstd_out [dev] f32 [batch * n_tokens]      the LayerNorm row statistics (as hs_layernorm_fwd)
 *   qkv_out  [dev] bf16 [batch, n_tokens, 3 * channels]  the qkv Linear's output (as hs_gemm_nt would have rounded it)
 *   attn_out [dev] bf16 [batch, n_tokens, channels]      hs_window_attn_fwd's `out`: the proj Linear's input
 *   lse_out  [dev] f32 [batch, num_heads, n_tokens]      hs_window_attn_fwd's `lse` (by shifted position)
 * HBM traffic per token: x in, out written, 5 C saved = 7 C * 2 B (+ 8 + 4 nH bytes of statistics) against 13 C * 2 B for
 * hs_layernorm_fwd -> hs_gemm_nt -> hs_window_attn_fwd -> hs_gemm_nt(HS_EPI_RESID), none of the saved tensors re-read in the forward.
 * norm2_gamma / norm2_beta / n2_out / mean2_out / rstd2_out (all five or none): the block's SECOND LayerNorm (:337) applied to `out`
 * in the same launch: n2_out [dev] bf16 [batch, n_tokens, channels] = LayerNorm(out) (what the MLP reads), its row statistics in
 * mean2_out / rstd2_out -- as hs_layernorm_fwd on `out` would have written them.
 * Same support set and argument meaning as hs_window_attn_module_fwd. */
int hs_window_attn_module_fwd_train(const void* x, void* out, void* xn_out, float* mean_out, float* rstd_out, void* qkv_out,
                                    void* attn_out, float* lse_out, const void* qkv_w, const float* qkv_b, const void* proj_w,
                                    const float* proj_b, const float* ln_gamma, const float* ln_beta, const float* bias,
                                    const float* head_scale, const int32_t* idx, int64_t roll, const uint8_t* labels,
                                    const float* norm2_gamma, const float* norm2_beta, void* n2_out, float* mean2_out, float* rstd2_out,
                                    int batch, int64_t n_tokens, int channels, int num_heads, int window_size, unsigned flags, int dtype,
                                    void* stream);

/* Backward of the same unit in one call: the gradients of out = [x +] proj(attention(qkv([LayerNorm](x)))) with respect to x and every
 * parameter, from dout and the tensors hs_window_attn_module_fwd_train saved.  Host-side chain of the kernels above and below on
 * `stream` (hs_linear_wgrad + hs_gemm_nt for proj, hs_window_attn_bwd, hs_linear_wgrad + hs_gemm_nt for qkv,
 * hs_add_layernorm_bwd for norm1 and the residual), not a fused kernel (DESIGN 4.6 says why).
 *   dout, x, xn, qkv, attn_out [dev] bf16 as written by / passed to the forward; mean, rstd, lse [dev] f32 likewise
 *   qkv_w_t [dev] bf16 [C, 3C], proj_w_t [dev] bf16 [C, C]: the TRANSPOSED weight copies (input-gradient products)
 *   ln_gamma NULL (v2 placement): x is the qkv Linear's input, xn / mean / rstd / dln_* are NULL, dx = dqkv W_q only
 *   dx [dev] bf16 [batch, n_tokens, C]; dqkv_w f32 [3C, C], dqkv_b f32 [3C] or NULL, dproj_w f32 [C, C], dproj_b f32 [C] or NULL,
 *   dln_gamma / dln_beta f32 [C], dbias f32 [nH, Ws, Ws] (NULL iff bias is), dhead_scale f32 [nH]: overwritten
 *   (accumulate == 0: every element is written, the buffers may hold anything) or added to (accumulate == 1: the callers' .grad
 *   buffers; micro-batches may reuse one workspace, the calls are ordered by the stream).  dx is written either way.
 *   accumulate takes 0 and 1 ONLY: the chained kernels take turns in one workspace region, so a sum deferred with HS_ACC_DEFER would
 *   find its partial records overwritten at the flush -- any other value returns HS_ERR_INVALID_ARG.
 *   workspace [dev] f32 [hs_window_attn_module_bwd_chain_workspace(...)]
 *   flags: HS_ATTN_COSINE, HS_ATTN_RESIDUAL as in the forward call.
 * Shapes: those of hs_window_attn_module_supported (bf16, window 64, head_dim 32, C = 96 or 128), n_tokens a positive multiple of 64,
 *   roll in [0, n_tokens), batch * n_tokens < 2^31.  REFUSED MEANS UNTOUCHED: every argument, alignment and shape condition of every
 *   chained kernel is checked before the first launch; a call that returns HS_ERR_INVALID_ARG / _UNSUPPORTED / _MISALIGNED has
 *   launched nothing, written no output and queued nothing for hs_reduce_flush. */
int64_t hs_window_attn_module_bwd_chain_workspace(int batch, int64_t n_tokens, int channels, int num_heads, int window_size);
int hs_window_attn_module_bwd_chain(const void* dout, const void* x, const void* xn, const float* mean, const float* rstd, const void* qkv,
                              const void* attn_out, const float* lse, const void* qkv_w_t, const void* proj_w_t, const float* ln_gamma,
                              const float* bias, const float* head_scale, const int32_t* idx, int64_t roll, const uint8_t* labels,
                              void* dx, float* dqkv_w, float* dqkv_b, float* dproj_w, float* dproj_b, float* dln_gamma, float* dln_beta,
                              float* dbias, float* dhead_scale, float* workspace, int accumulate, int batch, int64_t n_tokens, int channels,
                              int num_heads, int window_size, unsigned flags, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Forward and input-gradient product of the path's Linear layers with the elementwise step behind it fused into the
 * epilogue (bf16 activations; replaces `F.linear` + `nn.GELU` + `nn.Dropout` at models_torch/swin_hp_transformer.py:38-44
 * (Mlp.forward), :136/:172 (qkv, proj), :392 (PatchMerging.reduction), :425/:447 (expand), :772-775 (skip concat + Linear),
 * :785-788 (1x1 head) and their autograd input gradients):
 *     acc[m, n] = sum_k a[m, k] * b[n, k]   (+ sum_k a2[m, k] * b2[n, k]   when k2 > 0)
 *   a  [dev] bf16, row m at a + m*lda (k valid elements); b [dev] bf16 [n rows], row n at b + n*ldb: a weight exactly as
 *   nn.Linear stores it ([out, in]); for an input gradient pass the transposed bf16 copy of the weight.  The second segment
 *   contracts a second operand pair into the same accumulator: cat([x, skip], -1) @ W^T without the concatenation
 *   (b = W, b2 = W + k, ldb = ldb2 = k + k2).  bias [dev] f32[n] or NULL.  c, aux [dev] bf16 [m, n] contiguous.
 *   epilogue HS_EPI_BIAS : c = acc + bias
 *            HS_EPI_GELU : c = h = acc + bias (skipped when c == NULL), aux = dropout(gelu_erf(h), drop_p, seed) [written]
 *            HS_EPI_DGELU: c = acc * dropout_mask * gelu_erf'(aux)          (aux = the saved h [read]; bias ignored)
 *            HS_EPI_RESID: c = acc + bias + aux                              (aux = a residual term [read])
 *   The dropout mask is the one hs_gelu_fwd/bwd draw for the same (seed, element index m*n_cols + n).
 *   k, k2, lda, ldb multiples of 8; n a multiple of 4; dtype must be HS_BF16 (fp32 runs keep the library GEMM).
 * hs_gemm_nt_set_tile: measurement hook (0 = built-in choice, 1 = 128x128 tiles, 2 = 256x128 x 3 stages, 3 = 256x256 x 2
 * stages; any other value runs the 128x128 tiles).
 * hs_gemm_nt_tile_variant: the tile variant (1 / 2 / 3) a call with this shape and epilogue would launch now: the value forced by
 * hs_gemm_nt_set_tile or the built-in choice, and 2 in place of 3 where HS_EPI_DGELU / _RESID meet n % 8 != 0 (pure host code).
 * ---------------------------------------------------------------------------------------------- */
#define HS_EPI_BIAS 0
#define HS_EPI_GELU 1
#define HS_EPI_DGELU 2
#define HS_EPI_RESID 3
int hs_gemm_nt(const void* a, int64_t lda, const void* b, int64_t ldb, int k, const void* a2, int64_t lda2, const void* b2,
               int64_t ldb2, int k2, const float* bias, void* c, void* aux, int64_t m, int n, int epilogue, float drop_p,
               uint64_t seed, int dtype, void* stream);
int hs_gemm_nt_set_tile(int variant);
int hs_gemm_nt_tile_variant(int64_t m, int n, int k, int k2, int epilogue);

/* ------------------------------------------------------------------------------------------------
 * The library GEMM (hipBLASLt) in its full product form, for the Linear products the library runs faster than hs_gemm_nt
 * (long reductions: Mlp.fc2, models_torch/swin_hp_transformer.py:42, with the block's residual add :338 behind it):
 *     d[m, n] = sum_k a[m, k] * w[n, k] + bias[n] + c[m, n]            fp32 accumulation, one rounding to bf16
 *   a [dev] bf16 [m, k], w [dev] bf16 [n, k] (nn.Linear layout), c [dev] bf16 [m, n] or NULL (the plain product), d [dev] bf16 [m, n];
 *   all row-major, contiguous and 16-byte aligned; n, k multiples of 8.  bias [dev] [n] of bias_dtype (HS_BF16 or HS_F32) or NULL.
 *   d must not overlap a, w or c (HS_ERR_INVALID_ARG): c != d is the point -- the residual is read in the product's epilogue and
 *   the sum is written once, where torch.addmm first copies c into d in a pass of its own.
 * hipBLASLt is resolved at run time from the copy the process already holds (PyTorch's), else from the ROCm installation; there
 * is no link dependency.  hs_lib_gemm_supported: 1 where that succeeded and a device is visible, else 0 -- hs_lib_gemm_nt then
 * returns HS_ERR_UNSUPPORTED and the caller keeps the library product + separate add.  hs_lib_gemm_set_supported(0) turns the
 * path off for the process (tests, A/B runs), (1) on again.
 * State kept by the library: one hipBLASLt handle per device; one 32 MiB workspace per (device, stream), allocated by the first
 * call on that stream outside a capture and kept; the descriptors of every shape met.  A call on a capturing stream allocates
 * nothing and times nothing: it runs the remembered choice, and on a stream without a workspace a candidate that needs none.
 * Algorithm choice: up to 8 candidates of hipblasLtMatmulAlgoGetHeuristic; the first call of a class (bit_length(m), n, k, c given)
 * outside a capture runs each 1 + 3 times on the caller's stream and operands and remembers the fastest for the process and device.
 * hs_lib_gemm_pick reports that choice for the current device: *index its position among the candidates (-1: none yet), *solution
 * the library's solution index, name a text for records (any of the three may be NULL).  hs_lib_gemm_set_pick pins position
 * `index` for the class instead of a trial (data-parallel ranks take rank 0's; a position past the candidates runs candidate 0);
 * index -1 forgets the class.
 * ---------------------------------------------------------------------------------------------- */
int hs_lib_gemm_supported(void);
int hs_lib_gemm_set_supported(int on);
int hs_lib_gemm_nt(const void* a, const void* w, const void* bias, int bias_dtype, const void* c, void* d, int64_t m, int n, int k,
                   void* stream);
int hs_lib_gemm_pick(int64_t m, int n, int k, int has_c, int* index, int* solution, char* name, int name_len);
int hs_lib_gemm_set_pick(int64_t m, int n, int k, int has_c, int index);

/* ------------------------------------------------------------------------------------------------
 * Fisheye image -> HEALPix projection, the input pipeline in front of the model.  Replaces, per image, the
 * sampling of data/segmentation/project_on_s2.py:344-372; the coordinate table (u, v) of a calibration is built once on
 * the host (heal_swin_amd/projection.py, the reference's project_s2_points_to_img :141-183) and stays resident.
 *   hs_pix2ang_nest     [host] healpy.pixelfunc.pix2ang(nside, ipix, nest=True) (:350) for ipix = first .. first+count-1:
 *                       theta, phi [host] f64[count].
 *   hs_sample_bilinear_u8   sample_bilinear(img, rx, ry).astype(np.uint8) (:38-73, :361): img [dev] u8[batch, channels,
 *                       height, width]; rx (along height), ry (along width) [dev] f64[n]; out [dev] u8[batch, channels, n].
 *                       float64, the reference's operation order, no FMA contraction: bit-exact.  Integer coordinates give 0
 *                       (both of the reference's weights vanish), neighbours outside the image contribute 0.
 *   hs_sample_mask_u8   sample_mask(mask, rx, ry, background) (:76-80, :362): nearest pixel by round-half-to-even,
 *                       outside the image -> background.  mask [dev] u8[batch, height, width]; out [dev] u8[batch, n].
 * ---------------------------------------------------------------------------------------------- */
int hs_pix2ang_nest(int nside, int64_t first, int64_t count, double* theta, double* phi);
int hs_sample_bilinear_u8(const void* img, int batch, int channels, int height, int width, const double* rx, const double* ry,
                          int64_t n, void* out, void* stream);
int hs_sample_mask_u8(const void* mask, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                      int background, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-sample rotation augmentation of the projection (heal_swin_amd/projection.py: random_rotations, rotated_coords,
 * HPProjector(..., rotations=)).  The reference projects once, offline, and has no augmentation; here the sphere is re-sampled
 * differently for every sample of a batch by rotating the sampling coordinates, so a rotated sample costs one interpolation.
 *   hs_hp_rotated_coords  u, v [dev] f64[batch, count]: image coordinates of the nested pixels first_pix .. first_pix + count - 1
 *                       for each of `batch` samples.  Per (sample b, pixel p), in float64 without FMA contraction:
 *                         g = centre of p as a unit vector (the steps of hs_pix2ang_nest; z and sin theta formed directly),
 *                         d = M_b g, M_b = rot[9 b .. 9 b + 8] row-major ([dev]: a captured step may overwrite the matrices
 *                         between replays); any real matrix is accepted, the angles do not depend on |d|,
 *                         r = hypot(d.x, d.y), theta = atan2(r, d.z), cos phi = d.x / r, sin phi = d.y / r (1, 0 where r == 0),
 *                         rho = sum_{i = 1 .. poly_order} k[i - 1] theta^i,
 *                         u = rho cos phi + cx_offset + width / 2 - 1/2, v = rho sin phi aspect_ratio + cy_offset + height / 2 - 1/2
 *                       (project_s2_points_to_img, data/segmentation/project_on_s2.py:141-183).  Convention: output pixel p shows
 *                       the camera-frame direction M_b g_p, i.e. the map shows the scene rotated by M_b^-1.  With the identity
 *                       the result equals the host table of projection.py to rounding (about 1e-12 px), not bit for bit.
 *                       cam [host] is read during the call and travels by value.  HS_ERR_INVALID_ARG before any launch: nside
 *                       no power of two, [first_pix, first_pix + count) outside [0, 12 nside^2), batch outside 1 .. 65535,
 *                       poly_order outside 1 .. 8, width or height <= 0, null pointer.  count == 0 returns HS_OK.
 *   hs_sample_*_per_sample  hs_sample_bilinear_u8 / hs_sample_mask_u8 (and, below, hs_sample_bilinear_u8_f32 /
 *                       hs_sample_nearest_f32) with one coordinate row per sample: rx, ry [dev] f64[batch, n], sample b reads row
 *                       b (batch <= 65535).  Same argument lists, same kernels and arithmetic: with every row equal, the result
 *                       is the shared-table entry point's bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_fisheye_camera {
    double k[8];                                /* rho = sum k[i - 1] theta^i, i = 1 .. poly_order */
    double cx_offset, cy_offset, aspect_ratio;
    int poly_order, width, height;              /* 1 <= poly_order <= 8 (WoodScape: 4); the size of the image sampled */
} hs_fisheye_camera;
int hs_hp_rotated_coords(int nside, int64_t first_pix, int64_t count, const hs_fisheye_camera* cam, const double* rot, int batch,
                         double* u, double* v, void* stream);
int hs_sample_bilinear_u8_per_sample(const void* img, int batch, int channels, int height, int width, const double* rx,
                                     const double* ry, int64_t n, void* out, void* stream);
int hs_sample_mask_u8_per_sample(const void* mask, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                                 int background, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rotation of maps that already live on the sphere (heal_swin_amd/hp_rotate.py: rotated_interp, HPRotator): the augmentation
 * of a dataset that was projected once, offline, as the reference's are (hp_img / hp_mask read from .npz files,
 * data/segmentation/hp_datasets.py:92-98).  No frame is needed: output pixel p of sample b shows the SOURCE MAP at direction
 * d = M_b g_p (the convention of hs_hp_rotated_coords), resampled with HEALPix's get_interpol evaluated per (sample, pixel).
 *   hs_hp_rotated_interp  pix [dev] i32[batch, 4, count], wgt [dev] f64[batch, 4, count], nearest [dev] i32[batch, count] for the
 *                       nested pixels first_pix .. first_pix + count - 1.  Per (sample b, pixel p), in float64 without FMA:
 *                         g = centre of p as a unit vector (as in hs_hp_rotated_coords), d = M_b g, M_b = rot[9 b .. 9 b + 8]
 *                         row-major ([dev]); any real matrix is accepted,
 *                         theta = atan2(hypot(d.x, d.y), d.z) (0 for d = 0), phi = atan2(d.y, d.x) reduced to [0, 2 pi) with
 *                         HEALPix's fmodulo,
 *                         then the steps of hs_hp_interp_weights_nest (T_Healpix_Base::get_interpol, nested): ring_above, the
 *                         two bracketing rings with weights linear in phi, then linear in theta; above the first and below the
 *                         last ring the four polar pixels with a quarter of the missing ring's weight each; the same order of
 *                         the four pixels,
 *                         nearest = the pixel of largest weight, the first maximum in that order
 *                         (data/segmentation/project_on_s2.py:83-105, evaluation.hp_nearest_pix_idcs).
 *                       A non-finite component of d: pix -1, wgt 0, nearest -1.  Against hs_hp_interp_weights_nest at the same
 *                       direction the pixels are equal and the weights agree to rounding, except where the direction lies
 *                       within rounding of a ring or of a pixel boundary along a ring (there the other bracket is chosen; the
 *                       interpolated value is continuous across it).
 *   hs_hp_rotated_interp_host  the same inline function in a plain loop, every pointer [host]: the oracle of the two device
 *                       entry points.
 *   hs_hp_rotate        one launch, one thread per (sample, output pixel), the geometry evaluated once and applied to every plane
 *                       given; no table is written.  npix = base_pix nside^2 pixels per map, base_pix in 1 .. 12; a source index
 *                       idx is covered iff (uint64_t) idx < (uint64_t) npix, compared before every load.
 *                         img [dev] u8[batch, channels, npix] -> img_out: v = ((w0 v0 + w1 v1) + w2 v2) + w3 v3 in float64 without
 *                           FMA, an uncovered neighbour reads 0.0 (as hs_sample_bilinear_u8's neighbours outside the image);
 *                           the byte is rint(v) (half to even) clamped to [0, 255] -- not the frame sampler's truncation, so that
 *                           a direction on a pixel centre (top weight 1 - 1e-14) returns that pixel's byte,
 *                         labels [dev] u8[batch, npix] -> labels_out: labels[b, nearest], `background` where uncovered (classes
 *                           never mix),
 *                         depth [dev] f32[batch, npix] -> depth_out: depth[b, nearest] copied bit for bit (inf and NaN included),
 *                           depth_fill where uncovered.
 *                       Each plane is given by both pointers or by neither (NULL).
 * HS_ERR_INVALID_ARG before any launch: nside no power of two or above 8192 (the indices are int32; 2^29 is HEALPix's own
 * limit), [first_pix, first_pix + count) outside [0, 12 nside^2), npix not in {1 .. 12} nside^2, batch outside 1 .. 65535,
 * channels outside 1 .. 16 with img given, exactly one pointer of a pair, no plane, an output overlapping its input, background
 * outside 0 .. 255, a null rot / pix / wgt / nearest.  count == 0 returns HS_OK.
 * ---------------------------------------------------------------------------------------------- */
int hs_hp_rotated_interp(int nside, int64_t first_pix, int64_t count, const double* rot, int batch, int32_t* pix, double* wgt,
                         int32_t* nearest, void* stream);
int hs_hp_rotated_interp_host(int nside, int64_t first_pix, int64_t count, const double* rot, int batch, int32_t* pix, double* wgt,
                              int32_t* nearest);
int hs_hp_rotate(int nside, int64_t npix, const double* rot, int batch, const uint8_t* img, int channels, uint8_t* img_out,
                 const uint8_t* labels, uint8_t* labels_out, int background, const float* depth, float* depth_out, float depth_fill,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Equirectangular panoramas (ERP, the lat/long image) onto the sphere (heal_swin_amd/erp.py: ERPProjector; csrc/erp_project.hip,
 * csrc/hs_erp_device.h): the full-sphere data entry point, no counterpart in the reference.  Output pixel p of sample b shows the
 * panorama at direction d = M_b g_p (the convention of hs_hp_rotated_coords), M_b = rot[9 b .. 9 b + 8] row-major ([dev]; any
 * real matrix is accepted).  Per (sample b, pixel p), in float64 without FMA:
 *   g = centre of nested pixel p as a unit vector (as in hs_hp_rotated_coords), d = M_b g,
 *   theta = atan2(hypot(d.x, d.y), d.z), phi = atan2(d.y, d.x) reduced to [0, 2 pi) with HEALPix's fmodulo,
 *   x = phi width / (2 pi) - 0.5 (column), y = theta height / pi - 0.5 (row): column j is centred at longitude
 *   2 pi (j + 0.5) / width, row i at colatitude pi (i + 0.5) / height.
 *   frame [dev] u8 or f32 [batch, channels, height, width] (frame_kind HS_U8 / HS_F32) -> frame_out, the same type,
 *     [batch, channels, npix]: j0 = floor x, fx = x - j0, i0 = floor y, fy = y - i0; columns WRAP (ja = j0 mod width,
 *     jb = (j0 + 1) mod width, non-negative), rows CLAMP (ia, ib = i0, i0 + 1 clamped to [0, height - 1]);
 *     v = (1-fy) ((1-fx) v[ia,ja] + fx v[ia,jb]) + fy ((1-fx) v[ib,ja] + fx v[ib,jb]), in that order.  These are the proper
 *     bilinear weights, not hs_sample_bilinear_u8's (which mirror the reference's ceil - r / r - floor and give 0 at integer
 *     coordinates).  With supersample = s in {0, 1, 2} the value is the mean of the un-rounded v at the centres of the 4^s nested
 *     children p 4^s .. p 4^s + 4^s - 1 at nside 2^s, summed in ascending order and multiplied by the exact 2^(-2s).  u8: rint
 *     (half to even) clamped to [0, 255]; f32: the value cast to float, NaN propagates.
 *   labels [dev] u8[batch, height, width] -> labels_out [batch, npix]: the pixel at column floor(x + 0.5) mod width and row
 *     floor(y + 0.5) clamped to [0, height - 1], at the pixel's own centre whatever supersample is; classes never mix.
 *   depth [dev] f32[batch, height, width] -> depth_out [batch, npix]: that pixel's word copied (inf and NaN keep their bits).
 *   A non-finite component of d (of any child, for the frame): 0 (u8) or NaN (f32), `background`, depth_fill; no load is issued.
 * npix = base_pix nside^2, base_pix in 1 .. 12.  Each plane is given by both pointers or by neither (NULL).  One launch, one
 * thread per (sample, output pixel), the geometry evaluated once and applied to every plane given; no table is written, no LDS,
 * no atomics.  hs_erp_to_hp_host runs the same inline function in a plain loop, every pointer [host]: the kernel's oracle, equal
 * bit for bit, because the sine and cosine of the pixel centre, hypot and atan2 are evaluated in +, -, *, / and sqrt alone
 * (csrc/hs_erp_device.h; about 1 ulp from the math library's values, which differ between the device and the host in the last bit).
 * For a matrix so large or so small that the squares of d's components leave float64's range, theta is pi / 2, 0 or pi.
 * HS_ERR_INVALID_ARG before any launch: nside no power of two, supersample outside {0, 1, 2}, nside << supersample above 8192
 * (the nested indices are int32), npix not in {1 .. 12} nside^2, batch outside 1 .. 65535, height or width below 1 or height
 * width >= 2^31, exactly one pointer of a pair, no plane, with a frame another frame_kind or channels outside 1 .. 16, background
 * outside 0 .. 255, a null rot, an output overlapping an input or the matrices.
 * ---------------------------------------------------------------------------------------------- */
int hs_erp_to_hp(int nside, int64_t npix, const double* rot, int batch, int height, int width, int supersample, const void* frame,
                 int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out, int background,
                 const float* depth, float* depth_out, float depth_fill, void* stream);
int hs_erp_to_hp_host(int nside, int64_t npix, const double* rot, int batch, int height, int width, int supersample, const void* frame,
                      int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out, int background,
                      const float* depth, float* depth_out, float depth_fill);

/* ------------------------------------------------------------------------------------------------
 * Surround view: the frames of a rig of 1 .. 8 calibrated fisheye cameras fused onto one sphere (heal_swin_amd/surround.py:
 * SurroundProjector; csrc/surround_project.hip, csrc/hs_surround_device.h).  WoodScape's rig is four cameras (FV, RV, MVL, MVR)
 * with an extrinsic quaternion each; the reference projects one camera at a time, offline, and has no counterpart.  All cameras
 * share one image size height x width.  Per (sample b, pixel p), in float64 without FMA and without a math-library call:
 *   g = centre of nested pixel p as a unit vector; for every camera c = 0 .. n_cameras - 1 with present[b, c] != 0 ([dev]
 *   u8[batch, n_cameras]; NULL: all present), d = M[b, c] g with M = rot[(b n_cameras + c) 9 ..] row-major ([dev]); a camera whose d
 *   is not finite is skipped;
 *   r = sqrt(dx^2 + dy^2), theta = atan2(r, dz), cos phi = dx / r, sin phi = dy / r (1, 0 where r == 0); theta > max_theta[c]: not
 *   seen (max_theta is what keeps a non-monotonic polynomial from folding far directions back into the image);
 *   rho, u, v as in hs_hp_rotated_coords; SEEN iff -1/2 <= u < width - 1/2 and -1/2 <= v < height - 1/2 (the nearest image pixel
 *   lies inside the image);
 *   weight w = a e: a = 1 - theta / max_theta[c]; m = min(u + 1/2, width - 1/2 - u, v + 1/2, height - 1/2 - v);
 *   e = min(1, m / edge_feather) for edge_feather > 0, else 1.  The camera COUNTS iff it is seen and w > 0.
 * The pixel is covered iff some camera counts; the winner is the counting camera of largest w, the lowest c among equal weights.
 *   frame [dev] u8 or f32 [batch, n_cameras, channels, height, width] -> frame_out [batch, channels, npix]: per camera the bilinear
 *     value at (v, u), i0 = floor v, j0 = floor u, the expression of hs_erp_to_hp, rows AND columns clamped to the image.  blend 0:
 *     the winner's value.  blend 1: (sum_c w_c val_c) / (sum_c w_c) over the counting cameras in ascending c, un-rounded values.
 *     u8: rint (half to even) clamped to [0, 255]; f32: the value cast.  Uncovered: 0 (u8), NaN (f32).
 *   labels [dev] u8[batch, n_cameras, height, width] -> labels_out [batch, npix], depth [dev] f32[the same] -> depth_out: the
 *     winner's pixel at row rint(v), column rint(u) (half to even), copied (depth as a word: NaN and inf keep their bits);
 *     `background` / depth_fill where uncovered.  Depth is each camera's own range: the parallax between the cameras' centres is
 *     ignored, the rig is treated as one viewpoint.
 *   camera_out [dev] u8[batch, npix], nullable: the winner's index, 255 where uncovered.
 * Every matrix and present byte a thread needs is read before its first store; no load is issued for a camera that does not
 * count.  One launch, one thread per (sample, output pixel), no table, no LDS, no atomics; rig [host] is read during the call and
 * travels by value (under 1 KB).  hs_surround_to_hp_host runs the same inline function in a plain loop, every pointer [host]: the
 * kernel's oracle, equal bit for bit.
 * HS_ERR_INVALID_ARG before any launch: nside no power of two or above 8192, npix not in {1 .. 12} nside^2, batch outside
 * 1 .. 65535, a null rig or rot, n_cameras outside 1 .. 8, a camera with poly_order outside 1 .. 8 or a size other than height x
 * width, max_theta outside (0, pi] or not finite, edge_feather negative or not finite, blend outside {0, 1}, height or width
 * below 1 or height width >= 2^31, exactly one pointer of a pair, no plane, with a frame another frame_kind or channels outside
 * 1 .. 16, background outside 0 .. 255, an output overlapping an input, the matrices or the present bytes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_surround_rig {
    int n_cameras;                              /* 1 .. 8 */
    hs_fisheye_camera cam[8];                   /* the intrinsics; every width / height equals the call's */
    double max_theta[8];                        /* radians, in (0, pi] */
    double edge_feather;                        /* pixels, >= 0 */
    int blend;                                  /* 0 winner, 1 feather */
} hs_surround_rig;
int hs_surround_to_hp(int nside, int64_t npix, const hs_surround_rig* rig, const double* rot, const uint8_t* present, int batch, int height,
                      int width, const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out,
                      int background, const float* depth, float* depth_out, float depth_fill, uint8_t* camera_out, void* stream);
int hs_surround_to_hp_host(int nside, int64_t npix, const hs_surround_rig* rig, const double* rot, const uint8_t* present, int batch,
                           int height, int width, const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels,
                           uint8_t* labels_out, int background, const float* depth, float* depth_out, float depth_fill, uint8_t* camera_out);

/* ------------------------------------------------------------------------------------------------
 * Rotation ensembles at evaluation (heal_swin_amd/hp_ensemble.py: HPRotationEnsemble; csrc/hp_ensemble.hip): the way back of
 * hs_hp_rotate.  A sample is predicted under several rotations; each prediction, made on a frame that hs_hp_rotate rotated by M
 * (pixel q shows the scene at M g_q), is resampled onto the unrotated grid and accumulated there; the finish kernels average.
 * The caller passes rot = M^T [dev] f64[batch, 9] (the inverse of an orthogonal M), so unrotated pixel p reads the prediction at
 * direction M^T g_p through hs_hp_rotated_interp's function, unchanged; rot == NULL is the unrotated member (pixel p itself with
 * weight 1).  npix = base_pix nside^2.  A neighbour j of the four is TAKEN when it is covered ((uint64_t) pix_j < npix), when
 * valid[b, pix_j] != 0 if `valid` ([dev] u8[batch, npix], in the rotated frame, nullable) is given, and, for depth, when its value
 * is finite.  Weights are rounded to fp32 once; sums run over j = 0 .. 3 in order in fp32 without FMA.
 *   hs_hp_ensemble_add_seg    pred: logits HS_F32 / HS_BF16 (| HS_PRED_ROWS16), element (b, c, pixel) at b*stride_b + c*stride_k +
 *                       pixel*stride_p as in hs_seg_confusion, n_classes <= 16.  value_j = softmax(row_j) in fp32
 *                       (mode HS_ENSEMBLE_PROB) or row_j itself (HS_ENSEMBLE_LOGIT).  acc [dev] f32[batch, npix, KP], KP =
 *                       4 ceil(n_classes / 4), 16-byte aligned: acc[b, p, c] += sum_j w_j value_j[c] (classes >= n_classes: += 0);
 *                       wsum [dev] f32[batch, npix] += sum_j w_j.  accumulate == 0 stores instead of adding (the first member: no
 *                       zero fill is needed); with accumulate != 0 a pixel that took no neighbour is not written.
 *   hs_hp_ensemble_add_depth  pred: HS_F32 / HS_BF16, element (b, pixel) at b*stride_b + pixel*stride_p; acc, wsum [dev]
 *                       f32[batch, npix]: acc += sum_j w_j d_j, wsum += sum_j w_j.
 *   hs_hp_ensemble_finish_seg  preds [dev] u8[batch, npix] = argmax_c acc[b, p, c] (the first maximum, a NaN counts as the maximum,
 *                       as torch.max) where wsum[b, p] > min_weight, `background` elsewhere; probs (nullable) [dev] f32, element
 *                       (b, c, p) at b*stride_b + c*stride_k + p*stride_p = acc / wsum there, 0 elsewhere.
 *   hs_hp_ensemble_finish_depth  out [dev] f32[batch, npix] = acc / wsum where wsum > min_weight, NaN elsewhere.
 *   hs_hp_ensemble_add_seg_host, hs_hp_ensemble_add_depth_host  the same inline per-pixel functions in a plain loop, every
 *                       pointer [host]: the oracle of the device entry points (the exponential is the one call that differs:
 *                       v_exp_f32 of x log2(e) on the device, expf on the host; about 1e-7 on a probability).
 * One thread per (sample, unrotated pixel), no LDS, no atomics: bit-reproducible.  HS_ERR_INVALID_ARG before any launch: nside no
 * power of two or above 8192, npix not in {1 .. 12} nside^2, batch outside 1 .. 65535, n_classes outside 1 .. 16, another
 * prediction kind or mode, a negative stride, HS_PRED_ROWS16 rows that are not contiguous / aligned / padded, a null pred / acc /
 * wsum / preds / out, acc or wsum overlapping the predictions or each other, background outside 0 .. 255, a negative or NaN
 * min_weight; HS_ERR_MISALIGNED: acc not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define HS_ENSEMBLE_PROB 0
#define HS_ENSEMBLE_LOGIT 1
int hs_hp_ensemble_add_seg(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int n_classes,
                           int64_t stride_b, int64_t stride_k, int64_t stride_p, const uint8_t* valid, int mode, int accumulate, float* acc,
                           float* wsum, void* stream);
int hs_hp_ensemble_add_seg_host(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int n_classes,
                                int64_t stride_b, int64_t stride_k, int64_t stride_p, const uint8_t* valid, int mode, int accumulate,
                                float* acc, float* wsum);
int hs_hp_ensemble_add_depth(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int64_t stride_b,
                             int64_t stride_p, const uint8_t* valid, int accumulate, float* acc, float* wsum, void* stream);
int hs_hp_ensemble_add_depth_host(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int64_t stride_b,
                                  int64_t stride_p, const uint8_t* valid, int accumulate, float* acc, float* wsum);
int hs_hp_ensemble_finish_seg(int64_t npix, int batch, int n_classes, const float* acc, const float* wsum, float min_weight, int background,
                              uint8_t* preds, float* probs, int64_t stride_b, int64_t stride_k, int64_t stride_p, void* stream);
int hs_hp_ensemble_finish_depth(int64_t npix, int batch, const float* acc, const float* wsum, float min_weight, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation: HEALPix predictions scored and back-projected onto the fisheye image plane (heal_swin_amd/evaluation.py).
 * The tables of a calibration (nearest pixel, four interpolation pixels and weights per image-plane pixel) are built once on
 * the host; the per-batch work is the three gathers below.
 *   hs_hp_interp_weights_nest  [host] healpy.pixelfunc.get_interp_weights(nside, theta, phi, nest=True)
 *                       (data/segmentation/project_on_s2.py:95, :313; HEALPix C++ get_interpol): theta, phi [host] f64[n];
 *                       pix [host] i64[4][n], wgt [host] f64[4][n] in healpy's order.  phi is reduced to [0, 2 pi) first
 *                       (HEALPix fmodulo); theta outside [0, pi], NaN or an infinite phi -> HS_ERR_INVALID_ARG.
 * Predictions `pred` [dev] are logits (pred_kind HS_F32 / HS_BF16, n_classes <= 64, element (b, c, pixel) at
 * b*stride_b + c*stride_k + pixel*stride_p as in hs_seg_ce_fwd) whose class is torch.max(logits, 1)'s index (the first
 * maximum; a NaN counts as the maximum), or class ids (pred_kind HS_PRED_LABELS, uint8, element (b, pixel) at
 * b*stride_b + pixel*stride_p; stride_k unused).  npix = base_pix nside^2 HEALPix pixels per image; a table entry >= npix
 * (a pixel of the base pixels the model does not see) is "uncovered".
 *   hs_backproject_labels  project_hp_mask_back (:319-341): out [dev] u8[batch, n_out] = class at nearest[i], or
 *                       `background` (the reference's s2_bkgd_class) where uncovered.  nearest [dev] i32[n_out].
 *   hs_backproject_image   project_hp_img_back (:302-316, healpy get_interp_val): hp_img [dev] u8[planes, npix];
 *                       idx [dev] i32[4][n_out], wgt [dev] f64[4][n_out]; out [dev] f64[planes, n_out] =
 *                       ((w0 v0 + w1 v1) + w2 v2) + w3 v3 in float64 without FMA, uncovered pixels read 255.0 (the
 *                       reference's fill): bit-exact.
 *   hs_seg_confusion    the confusion matrix of torchmetrics 0.3.2 (bincount(target * K + pred), rows = target, columns =
 *                       prediction; models_lightning/segmentation/model_lightning_swin_hp.py:47-55), ADDED into conf [dev]
 *                       i64[n_classes, n_classes].  nearest == NULL: HEALPix domain, target [dev] u8[batch, npix].  Otherwise
 *                       image plane (evaluation/hp_pred_writers.py:110-222): the prediction of pixel i is read at nearest[i],
 *                       target [dev] u8[batch, n_out], and uncovered pixels count as class `uncovered` (back-projected
 *                       metrics) or are skipped when uncovered = -1 (evaluation/custom_metrics.py:25-59, HPMaskedIoU).
 *                       Pixels with target >= n_classes (or a label prediction >= n_classes) are not counted but added to
 *                       bad [dev] i64[2] (targets, predictions), on which the caller raises as torchmetrics does.  Integer
 *                       atomics only: exact and deterministic.
 * ---------------------------------------------------------------------------------------------- */
#define HS_PRED_LABELS 2
#define HS_PRED_ROWS16 4 /* or'ed into HS_F32 / HS_BF16: stride_k == 1 and every pixel's logits row is 16-byte aligned and may be
                            read up to the next multiple of 16 bytes (the model's padded rows); the rows are then read with
                            16-byte loads */
int hs_hp_interp_weights_nest(int nside, const double* theta, const double* phi, int64_t n, int64_t* pix, double* wgt);
int hs_backproject_labels(const void* pred, int pred_kind, int64_t batch, int64_t npix, int n_classes, int64_t stride_b,
                          int64_t stride_k, int64_t stride_p, const int32_t* nearest, int64_t n_out, int background, uint8_t* out,
                          void* stream);
int hs_backproject_image(const uint8_t* hp_img, int64_t planes, int64_t npix, const int32_t* idx, const double* wgt, int64_t n_out,
                         double* out, void* stream);
int hs_seg_confusion(const void* pred, int pred_kind, int64_t batch, int64_t npix, int n_classes, int64_t stride_b, int64_t stride_k,
                     int64_t stride_p, const int32_t* nearest, int64_t n_out, const uint8_t* target, int uncovered, int64_t* conf,
                     int64_t* bad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth evaluation (heal_swin_amd/depth_evaluation.py, csrc/depth_eval.hip): point clouds, Chamfer nearest neighbours, the
 * depth error metrics and the float back-projection.  Depth values are read in place: kind HS_F32 / HS_BF16, element (b, i) of
 * n = rows * width at b*stride_b + (i / width)*stride_h + (i % width)*stride_w (HEALPix data: width = n, stride_h unused).
 *   hs_depth_points     create_point_cloud_from_depth_mask (heal_swin/utils/depth_utils.py:465-539) and the kept set of
 *                       ChamferDistance.update (evaluation/custom_metrics.py:539-561).  Pixel i of sample b is kept when its depth
 *                       is finite, differs from every background[0 .. n_background) (<= 4) and, if foreground [dev] u8 (element
 *                       b*fg_stride_b + i) is given, foreground is nonzero.  Kept points, in pixel order, sample after sample:
 *                       points [dev] f32[batch * n][3] rows offsets[b] .. offsets[b+1] = fp32(d * dir[:, i]) (float64 product),
 *                       dir [dev] f64[3][n] the rotated unit directions; offsets [dev] i64[batch + 1].  Rows past offsets[batch]
 *                       are not written.  workspace [dev]: hs_depth_points_workspace(batch, n) bytes.  Deterministic (counts,
 *                       one scan, writes).
 *   hs_chamfer_nn       for every sample s, clouds a (rows a_off[s] .. a_off[s+1] of a [dev] f32[a_rows][3]) and b:
 *                       dist_a[i] = min_j |a_i - b_j|^2, dist_b[j] = min_i |a_i - b_j|^2 (fp32, dx*dx + dy*dy + dz*dz from the
 *                       coordinate differences, FMA-chained), idx_a / idx_b [dev] i64 the lowest index within the other cloud
 *                       attaining it (both NULL: distances only).  a_max / b_max bound the points of one sample (grid size; the
 *                       offsets are not read on the host).  Rows of a sample whose other cloud is empty, and rows past the last
 *                       cloud, get NaN and -1.  term [dev] f64[batch] (optional) = mean(dist_a) + mean(dist_b) of the sample,
 *                       NaN when a cloud is empty.  splits: target-range workgroups per query block (0: automatic); the results
 *                       are bit-identical for every value.  workspace [dev]: 8 * (a_rows + b_rows) bytes.
 *   hs_depth_metrics    one pass over pred (kind HS_F32 / HS_BF16 / HS_F64; the mean at channel 0, the log variance at +stride_c
 *                       when use_logvar) and target (same layout, strides t_stride_*), ADDING the HS_DEPTH_NSUMS sums below into
 *                       state [dev] f64[HS_DEPTH_NSUMS] (custom_metrics.py:62-468; selections there).  ranges [host] f32[2][n_ranges]
 *                       (lo, hi) pairs, n_ranges <= 8.  partial [dev] f64[hs_depth_metrics_partials(batch * n)][HS_DEPTH_NSUMS]
 *                       scratch.  Per-element values in the reference's compute type, sums in float64 in a fixed order.
 *   hs_backproject_depth  project_depth_hp_mask_back(..., s2_bkgd_class=nan) (data/depth_estimation/project_depth_on_s2.py:370-386):
 *                       values (b, p) at b*stride_b + p*stride_p, out [dev] f64[batch, n_out] = ((w0 v0 + w1 v1) + w2 v2) + w3 v3
 *                       with v = NaN where idx >= npix (hs_backproject_image's tables and order).
 * ---------------------------------------------------------------------------------------------- */
#define HS_F64 3
#define HS_DS_N 0       /* pred and target finite: count */
#define HS_DS_SE 1      /*   sum (p - t)^2 */
#define HS_DS_AE 2      /*   sum |p - t| */
#define HS_DS_MEAN_SE 3 /*   sum (total_mean - t)^2 */
#define HS_DS_MEAN_AE 4 /*   sum |total_mean - t| */
#define HS_DS_PRED 5    /*   sum p */
#define HS_DS_SIL_N 6   /*   and p > 0, t > 0: count */
#define HS_DS_SIL_D 7   /*     sum (log t - log p) */
#define HS_DS_SIL_D2 8  /*     sum (log t - log p)^2 */
#define HS_DS_INV_N 9   /* 1 / (0.001 p), 1 / (0.001 t) finite: count */
#define HS_DS_INV_SE 10 /*   sum of their squared difference */
#define HS_DS_STD_N 11  /* target not NaN and not +inf: count */
#define HS_DS_STD 12    /*   sum sqrt(exp(log_var)) */
#define HS_DS_RANGE 13  /* 2 r, 2 r + 1: count and sum (p - t)^2 of the finite pairs with lo_r <= t < hi_r */
#define HS_DEPTH_NSUMS 29
int64_t hs_depth_points_workspace(int64_t batch, int64_t n);
int hs_depth_points(const void* depth, int kind, int64_t batch, int64_t n, int64_t width, int64_t stride_b, int64_t stride_h,
                    int64_t stride_w, const uint8_t* foreground, int64_t fg_stride_b, const float* background, int n_background,
                    const double* dir, void* workspace, float* points, int64_t* offsets, void* stream);
int hs_chamfer_nn(const float* a, const int64_t* a_off, int64_t a_rows, int64_t a_max, const float* b, const int64_t* b_off,
                  int64_t b_rows, int64_t b_max, int64_t batch, int splits, void* workspace, float* dist_a, float* dist_b,
                  int64_t* idx_a, int64_t* idx_b, double* term, void* stream);
int64_t hs_depth_metrics_partials(int64_t total);
int hs_depth_metrics(const void* pred, int pred_kind, int64_t batch, int64_t n, int64_t width, int64_t stride_b, int64_t stride_c,
                     int64_t stride_h, int64_t stride_w, const void* target, int target_kind, int64_t t_stride_b, int64_t t_stride_h,
                     int64_t t_stride_w, int use_logvar, double total_mean, const float* ranges, int n_ranges, double* partial,
                     double* state, void* stream);
int hs_backproject_depth(const void* pred, int kind, int64_t batch, int64_t npix, int64_t stride_b, int64_t stride_p, const int32_t* idx,
                         const double* wgt, int64_t n_out, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The flat baseline on the sphere (heal_swin_amd/flat_evaluation.py, csrc/flat_eval.hip): depth predictions of the image plane
 * sampled at n HEALPix pixels through the tables of FlatToHPProjector (negative Pad, Resize and
 * project_depth_on_s2.sample_mask(..., s2_bkgd_class=nan) composed on the host; evaluation/flat_depth_pred_writers.py:216-239).
 * The prediction is read in place: kind HS_F32 / HS_BF16, element (b, channel c, source pixel q) at b*stride_b + c*stride_c +
 * q*stride_p, q < n_src (an NCHW map: stride_p = 1; the model's head rows: stride_c = 1).  Give EITHER nearest [dev] i32[n], the
 * source pixel of every HEALPix pixel, OR idx [dev] i32[4][n] (taps y0x0, y0x1, y1x0, y1x1) with wgt [dev] f32[4][n] (h0, h1, w0,
 * w1); the other pointers NULL.  A HEALPix pixel whose table entry (any tap) lies outside [0, n_src) is uncovered and reads NaN.
 *   hs_flat_depth_to_hp      out [dev] f32[batch][n]: nearest values copied bit for bit; bilinear values
 *                            h0*(w0*p00 + w1*p01) + h1*(w0*p10 + w1*p11) in fp32 without contraction (torch's order).
 *   hs_depth_metrics_gather  hs_depth_metrics with that value as the prediction (the log variance, channel 1, gathered the same
 *                            way when use_logvar) against target (b, i) at b*t_stride_b + i*t_stride_p (HS_F32 / HS_BF16), ADDING
 *                            into state; partial [dev] f64[hs_depth_metrics_partials(batch * n)][HS_DEPTH_NSUMS] scratch.  Same
 *                            per-element rules, lane map and merge order as hs_depth_metrics: the state is bit-identical to
 *                            hs_depth_metrics on hs_flat_depth_to_hp's output, which is never written here.
 * ---------------------------------------------------------------------------------------------- */
int hs_flat_depth_to_hp(const void* pred, int kind, int64_t batch, int64_t n_src, int64_t stride_b, int64_t stride_p, const int32_t* nearest,
                        const int32_t* idx, const float* wgt, int64_t n, float* out, void* stream);
int hs_depth_metrics_gather(const void* pred, int pred_kind, int64_t batch, int64_t n_src, int64_t stride_b, int64_t stride_c, int64_t stride_p,
                            const int32_t* nearest, const int32_t* idx, const float* wgt, int64_t n, const void* target, int target_kind,
                            int64_t t_stride_b, int64_t t_stride_p, int use_logvar, double total_mean, const float* ranges, int n_ranges,
                            double* partial, double* state, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The depth data path (heal_swin_amd/depth_data.py): the per-frame sampling of data/depth_estimation/project_depth_on_s2.py
 * (project_depth_dataset_hp :389-440, against hs_sample_*_u8's coordinate tables; the same kernels as hs_sample_*_u8,
 * csrc/projection.hip), the target transforms of the depth datasets and Lightning module, and compute_depth_stats.py's statistics
 * (csrc/depth_data.hip).
 *   hs_sample_bilinear_u8_f32  sample_bilinear(img, rx, ry).astype(np.float32) (:48-77): hs_sample_bilinear_u8's float64
 *                       arithmetic rounded once to float32, NaN where a coordinate is not finite.  out [dev] f32[batch, channels, n].
 *   hs_sample_nearest_f32  sample_mask(depth, rx, ry, background) (:80-84): src [dev] f32[batch, height, width] -> out [dev]
 *                       f32[batch, n], nearest pixel by round-half-to-even, values copied exactly, background outside the image.
 *   hs_depth_target     out[b * out_stride_b + i * out_stride_p] = op(in[b * in_stride_b + i * in_stride_p]) for b < batch (<= 65535),
 *                       i < n; out may equal in.  Forward (no HS_DT_INVERSE): 0 -> inf if HS_DT_ZERO_BKG, 1000 -> inf if
 *                       HS_DT_1000_BKG, the transform (HS_DT_LOG: log; HS_DT_INV: inverse_mask, utils/depth_utils.py:60-72), then
 *                       (x - shift) / scale if HS_DT_AFFINE.  Inverse: x * scale + shift if HS_DT_AFFINE, then exp / inverse_mask.
 *                       float32, transcendentals as fp32(f(double x)).
 *   hs_depth_stats_update  ADDS one float32 array depth [dev] f32[n] (raw depths) into state [dev] (HS_DEPTH_STATS_WORDS words:
 *                       int64 counts HS_DSTAT_*, then float64 mean, M2, min, max of the finite transformed values and the max of
 *                       those whose raw value is not 1000).  use_masking drops raw 1000s (they are still counted as background);
 *                       HS_DT_LOG: fp32(log x), HS_DT_INV: fp32(1 / x) (the script's plain reciprocal).  partial [dev]
 *                       HS_DEPTH_STATS_WORDS * hs_depth_stats_partials(n) words of scratch.  Deterministic: no float atomics.
 *   hs_depth_stats_merge  state (+)= states[0], ..., states[count - 1] (each HS_DEPTH_STATS_WORDS words, [dev]), in that order.
 *                       A state starts as zero counts, mean = M2 = 0, min = +inf, max = fg max = -inf.
 *   hs_histogram_update  compute_depth_stats.py's np.histogram: ADDS the counts of one float32 array depth [dev] f32[n] into
 *                       counts [dev] i64[bins], 1 <= bins <= HS_HISTOGRAM_MAX_BINS.  The value counted is the one
 *                       hs_depth_stats_update forms (same transform, same use_masking), widened to float64: bin i holds
 *                       edges[i] <= v < edges[i + 1], the last bin is closed at edges[bins]; NaN, +-inf and values outside
 *                       [edges[0], edges[bins]] are dropped.  edges [dev] f64[bins + 1], increasing (numpy's own
 *                       np.histogram_bin_edges): the bin is estimated arithmetically and corrected against the table.
 *                       Integer adds only: the counts do not depend on the order of arrival.
 * ---------------------------------------------------------------------------------------------- */
#define HS_HISTOGRAM_MAX_BINS 4096
#define HS_DT_NONE 0
#define HS_DT_LOG 1
#define HS_DT_INV 2
#define HS_DT_ZERO_BKG 1
#define HS_DT_1000_BKG 2
#define HS_DT_AFFINE 4
#define HS_DT_INVERSE 8
#define HS_DSTAT_TOTAL 0      /* raw values seen */
#define HS_DSTAT_BACKGROUND 1 /* raw values == 1000 */
#define HS_DSTAT_VALUES 2     /* values kept (all, or the non-1000 ones with use_masking) */
#define HS_DSTAT_FINITE 3     /* kept values finite after the transform */
#define HS_DSTAT_POSINF 4     /*   +inf */
#define HS_DSTAT_NEGINF 5     /*   -inf */
#define HS_DSTAT_NAN 6        /*   NaN */
#define HS_DSTAT_FG_VALUES 7  /* kept values whose raw value is not 1000 */
#define HS_DSTAT_FG_POSINF 8  /*   +inf */
#define HS_DSTAT_FG_NAN 9     /*   NaN */
#define HS_DSTAT_NCOUNTS 10
#define HS_DEPTH_STATS_WORDS 15
int hs_sample_bilinear_u8_f32(const void* img, int batch, int channels, int height, int width, const double* rx, const double* ry,
                              int64_t n, float* out, void* stream);
int hs_sample_nearest_f32(const float* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                          float background, float* out, void* stream);
/* rx, ry [dev] f64[batch, n], one row per sample (see hs_hp_rotated_coords above) */
int hs_sample_bilinear_u8_f32_per_sample(const void* img, int batch, int channels, int height, int width, const double* rx,
                                         const double* ry, int64_t n, float* out, void* stream);
int hs_sample_nearest_f32_per_sample(const float* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                                     float background, float* out, void* stream);
int hs_depth_target(const float* in, int64_t in_stride_b, int64_t in_stride_p, float* out, int64_t out_stride_b, int64_t out_stride_p,
                    int64_t batch, int64_t n, int flags, int transform, float shift, float scale, void* stream);
int64_t hs_depth_stats_partials(int64_t n);
int hs_depth_stats_update(const float* depth, int64_t n, int transform, int use_masking, int64_t* partial, int64_t* state, void* stream);
int hs_depth_stats_merge(const int64_t* states, int count, int64_t* state, void* stream);
int hs_histogram_update(const float* depth, int64_t n, int transform, int use_masking, const double* edges, int bins, int64_t* counts,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Order statistics of rows (heal_swin_amd/order_stats.py): MeanSTDMedian's torch.median (evaluation/custom_metrics.py) without
 * the sort.
 *   hs_select_rows      out[r] = the k-th smallest (0-based) of x[r * row_stride .. r * row_stride + n), r < rows (<= 65535),
 *                       0 <= k < n < 2^31, row_stride >= n, in torch.sort's order: -inf < finite < +inf < NaN, every NaN
 *                       (either sign, any payload) last, -0.0 and +0.0 equal (either may be returned).  nan_propagates: a row
 *                       that holds a NaN gives NaN (torch.median's rule; torch.kthvalue's is nan_propagates = 0).  x [dev] f32,
 *                       4-byte aligned: a scalar head and tail around the 16-byte body of every row.  Radix select, four 8-bit
 *                       digits from the top, on the order-preserving key (NaN -> 0xFFFFFFFF, else bits ^ (sign ? 0xFFFFFFFF :
 *                       0x80000000)): `splits` workgroups per row (0: chosen from rows and n) count the digit of the elements
 *                       that match the prefix and add their bins into workspace with integer atomics; every workgroup of the
 *                       next pass finds prefix and rank from those bins itself.  Four pass launches and one that writes out;
 *                       the result is bit-identical for every `splits` and arrival order.  workspace [dev]
 *                       hs_select_rows_workspace(rows) bytes, zeroed in the call on `stream`.  Never waits for the device; can
 *                       be captured in a graph (a replay selects from the current contents of x).
 * ---------------------------------------------------------------------------------------------- */
int64_t hs_select_rows_workspace(int rows);
int hs_select_rows(const float* x, int rows, int64_t n, int64_t row_stride, int64_t k, int nan_propagates, int splits, void* workspace,
                   float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decoder tail: LayerNorm(C) of FinalPatchExpand_X4 + the 1x1 class head in one pass, so that the normalised
 * [B, 4 N0, C] tensor is never written.  Replaces `self.norm(x)` (models_torch/swin_hp_transformer.py:448-452) followed by
 * `self.output(x)` (:756-761, :785-788) and their backward.  bf16 rows, C in {64, 96, ..., 256}, <= 16 classes.
 *   y [dev] bf16[rows, C] (the expanded rows); logits [dev] bf16[rows, 16] (columns >= n_classes are 0).
 *   forward : wfold [dev] bf16[32, C] = gamma * W[k, :] (rows >= n_classes zero), bvec [dev] f32[32] = sum_c beta_c W[k, c];
 *             mean, rstd [dev] f32[rows] are saved for the backward.
 *   backward: afold [dev] bf16[C, 16] = (gamma * W)^T (columns >= n_classes zero); dlogits [dev] bf16[rows, 16];
 *             dy [dev] bf16[rows, C] = LayerNorm input gradient; dprime [dev] bf16[rows, 16] = dlogits * rstd;
 *             partials [dev] f32[hs_ln_head_partials(rows), 32]: per-wave sums u[k] = sum dlogits (0..15) and
 *             t[k] = sum dprime * mean (16..31).  With X = hs_linear_wgrad(dprime, y) - t:  dW = gamma X + beta u,
 *             dgamma_c = sum_k W X, dbeta_c = sum_k W u   (heal_swin_amd/ops/tail.py:LnHeadFn).
 *   logits_dtype: HS_BF16 (32-byte rows) or HS_F32 (64-byte rows: the logits keep their fp32 accumulator value and xhat enters the
 *             head product as hi + lo; dlogits is then read as fp32 too) -- the decoder tail's roundings are not averaged by
 *             anything downstream and dominate the bf16 logit error, see csrc/ln_head.hip.
 * ---------------------------------------------------------------------------------------------- */
int hs_ln_head_supported(int width, int n_classes, int dtype);
int64_t hs_ln_head_partials(int64_t rows);
int hs_ln_head_fwd(const void* y, const void* wfold, const float* bvec, void* logits, float* mean, float* rstd, int64_t rows,
                   int width, int dtype, int logits_dtype, void* stream);
int hs_ln_head_bwd(const void* y, const float* mean, const float* rstd, const void* dlogits, const void* afold, void* dy,
                   void* dprime, float* partials, int64_t rows, int width, int dtype, int logits_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 x 3 products for fp32 activations (the reference trains in fp32, training/train_config.py:95).  hs_split_bf16x3 writes, for
 * fp32 x [rows, k], the bf16 matrix [rows, 3 k] = [hi | hi | lo] (mode 0: activation side) or [hi | lo | hi] (mode 1: weight side),
 * hi = bf16(x), lo = bf16(x - hi): a bf16 GEMM of depth 3 k over a mode-0 and a mode-1 operand with fp32 accumulation equals
 * a_hi b_hi + a_hi b_lo + a_lo b_hi, i.e. the fp32 product to ~1e-5 relative, at 3/16 of the fp32-MFMA time (csrc/split3.hip).
 * hs_linear_wgrad_ld is hs_linear_wgrad (bf16) on the column blocks [ycol0, ycol0 + n_out) / [xcol0, xcol0 + k_in) of matrices with row
 * strides ldy / ldx (elements, multiples of 8; dy / x point to the matrices' first elements): the hi / lo blocks of two mode-0 matrices feed the three weight-gradient products (accumulate = 1 on the second and third).
 * ---------------------------------------------------------------------------------------------- */
int hs_split_bf16x3(const float* x, void* out, int64_t rows, int k, int mode, void* stream);
/* GELU fused with the split: out3 [rows, 3 k] bf16 = [hi | hi | lo] of dropout(gelu_erf(x)) (dy == NULL: the forward, x the
 * pre-activation) or of dy * dropout_mask * gelu_erf'(x) (the backward), x / dy [rows, k] fp32 -- for tensors that only
 * bf16 x 3 products read (the MLP hidden activation and its gradient): no fp32 copy is written.  Same dropout mask as
 * hs_gelu_fwd / hs_gelu_bwd for (seed, element index row * k + column).
 * Both entry points: k a positive multiple of 4; x / dy 16-byte aligned, out 8-byte aligned ("Pointer alignment"). */
int hs_gelu_split3(const float* dy, const float* x, void* out3, int64_t rows, int k, float drop_p, uint64_t seed, void* stream);
int hs_linear_wgrad_ld(const void* dy, int64_t ldy, int64_t ycol0, const void* x, int64_t ldx, int64_t xcol0, float* dw, float* dbias,
                       float* workspace, int64_t rows, int n_out, int k_in, int accumulate, void* stream);

/* The whole decoder tail forward in one launch: FinalPatchExpand_X4's Linear(C -> 4 C) (models_torch/swin_hp_transformer.py:442-447),
 * the 'b n (p c) -> b (n p) c' view (:449), its LayerNorm(C) (:450-452) and the 1x1 class head (:785-788).  LayerNorm reads the fp32
 * accumulators of the expand product, xhat enters the head as hi + lo, the logits leave in fp32: of the tail's four bf16 roundings
 * only the input's remains (csrc/expand_ln_head.hip).  bf16, 4 children, C in {64, 96, 128} (the expand weight lives in LDS).
 *   xn [dev] bf16[tokens, C] (the norm_up output), xn_lo [dev] bf16[tokens, C] or NULL: its rounding remainder (hs_layernorm_fwd_ex lo_out) --
 *   with it the expand product takes its input as hi + lo and the tail has NO bf16 rounding between norm_up and the logits;
 *   wexp [dev] bf16[4 C, C] as nn.Linear stores it; wfold [dev] bf16[64, C]: rows 0..31 = gamma * W[k, :] rounded to bf16 (rows >=
 *   n_classes zero), rows 32..63 its rounding remainder; bvec as for hs_ln_head_fwd;
 *   logits [dev] f32[4 tokens, 16]; y [dev] bf16[4 tokens, C] + mean, rstd [dev] f32[4 tokens]: what the backward (hs_ln_head_bwd on y,
 *   then the Linear's gradients) needs -- all three NULL for a forward without gradient, in which case the expanded tensor never exists. */
int hs_expand_ln_head_supported(int width, int children, int n_classes, int dtype);
int hs_expand_ln_head_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, void* y, float* logits,
                          float* mean, float* rstd, int64_t tokens, int width, int children, int dtype, void* stream);

/* The tail WITH the segmentation caller's loss (nn.CrossEntropyLoss(weight=...)(logits, masks.long()),
 * models_lightning/segmentation/model_lightning_swin_hp.py:39-45, :104-111): the forward kernel above additionally takes the pixel
 * labels, forms the weighted cross-entropy of every row from the fp32 logits it holds in registers and writes per-wavefront partial
 * sums; with logits == NULL the [4 tokens, 16] fp32 logits tensor is never written (training: 403 MB at nside 256, batch 8, plus the
 * loss kernels' 3 passes over it).  The backward recomputes the row's logits from the saved expanded rows y, forms
 * dlogits = scale w[label] (softmax - onehot) in registers and continues as hs_ln_head_bwd (same outputs).
 *   labels [dev] u8[4 tokens] in pixel order (row = 4 token + child); ids >= n_classes carry weight 0;
 *   class_weights [dev] f32[n_classes] or NULL (all ones);
 *   loss_partials [dev] f32[4 * hs_expand_ln_head_blocks(tokens), 2]: sums of w (lse - logit_label) and of w per wavefront:
 *                 loss = sum(col 0) / sum(col 1)  (the reference's weighted mean);
 *   backward: scale [dev] f32[1] = dloss / sum(col 1); wfold [dev] bf16[64, C] and bvec [dev] f32[32] as for the forward but with row
 *             blocks 4..7 and 8..11 EXCHANGED (heal_swin_amd/ops/tail.py:_fold_head_ce; csrc/ln_head.hip says why); afold, dy, dprime,
 *             partials as for hs_ln_head_bwd.  bf16, C in {64, 96, 128}. */
int64_t hs_expand_ln_head_blocks(int64_t tokens);
int hs_expand_ln_head_ce_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, const uint8_t* labels,
                             const float* class_weights, int n_classes, void* y, float* logits, float* mean, float* rstd,
                             float* loss_partials, int64_t tokens, int width, int children, int dtype, void* stream);
/* ... and WITH the caller's whole shared_step (model_lightning_swin_hp.py:104-111: `preds = torch.max(outputs, 1)`, the loss, IoU /
 * Accuracy on (preds, masks)): hs_expand_ln_head_ce_fwd's arguments, loss partials and saved tensors (bit for bit: the same
 * arithmetic in the same order; the backward is hs_ln_head_ce_bwd), plus, each optional (NULL: not produced),
 *   preds   [dev] u8[4 tokens]: the row's class id as torch.max(logits, 1) gives it on the fp32 logits (first maximal class of
 *           0..n_classes-1; a NaN counts as the maximum, the first NaN wins); 4-byte aligned;
 *   confmat [dev] i64[n_classes, n_classes]: confmat[label, pred] += 1 per row (hs_seg_confusion's matrix; integer atomics: exact
 *           and deterministic); rows whose label is >= n_classes stay out and are counted in
 *   bad     [dev] i64[2]: bad[0] += their number (required with confmat; [1] is untouched: predictions are always < n_classes).
 * No logits are needed for any of them (logits == NULL as above); y, mean, rstd NULL is the validation form.  No host
 * synchronisation, no allocation: capturable in a HIP graph.  HS_ERR_INVALID_ARG if one wavefront could own 2^32 rows. */
int hs_expand_ln_head_ce_step_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec,
                                  const uint8_t* labels, const float* class_weights, int n_classes, void* y, float* logits, float* mean,
                                  float* rstd, float* loss_partials, uint8_t* preds, int64_t* confmat, int64_t* bad, int64_t tokens,
                                  int width, int children, int dtype, void* stream);
int hs_ln_head_ce_bwd(const void* y, const float* mean, const float* rstd, const uint8_t* labels, const float* class_weights,
                      const float* scale, int n_classes, const void* wfold, const float* bvec, const void* afold, void* dy, void* dprime,
                      float* partials, int64_t rows, int width, int dtype, void* stream);

/* The tail WITH the depth caller's loss (hs_depth_loss_fwd's kinds and semantics): the same forward kernel forms the depth term of
 * every row from the fp32 head outputs it holds (channel 0 = mean, channel 1 = log variance for HS_DEPTH_LOGVAR) and writes
 * per-wavefront (sum, kept count) partials; with logits == NULL the [4 tokens, 16] fp32 rows are never written.  The backward
 * recomputes the head outputs from the saved y, forms dpred in registers (exactly 0 at rows whose target is infinite) and continues
 * as hs_ln_head_bwd.  n_out (the head's f_out) is 1 or 2: HS_DEPTH_HUBER needs 1, HS_DEPTH_LOGVAR 2.
 *   target [dev] f32[4 tokens] in pixel order (row = 4 token + child);
 *   loss_partials [dev] f32[4 * hs_expand_ln_head_blocks(tokens), 2]: loss = sum(col 0) / sum(col 1);
 *   wfold, bvec as for hs_expand_ln_head_fwd (unpermuted: the exchange of hs_ln_head_ce_bwd moves classes 4..11 only, so a head of
 *   one or two channels sits in the same accumulator registers with either order);
 *   backward: scale [dev] f32[1] = dloss / sum(col 1); afold, dy, dprime, partials as for hs_ln_head_bwd.  bf16, C in {64, 96, 128}. */
int hs_expand_ln_head_depth_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, const float* target,
                                int kind, float huber_delta, int n_out, void* y, float* logits, float* mean, float* rstd, float* loss_partials,
                                int64_t tokens, int width, int children, int dtype, void* stream);
/* ... and WITH the depth caller's whole shared_step (models_lightning/depth_estimation/model_lightning_depth_swin_hp.py:132-159: the
 * loss in the normalised space, unnormalize_and_retransform of prediction and target, the depth metrics on them):
 * hs_expand_ln_head_depth_fwd's arguments, loss partials and saved tensors (bit for bit: the same arithmetic in the same order; the
 * backward is hs_ln_head_depth_bwd), plus
 *   flags, transform, shift, scale   hs_depth_target's INVERSE chain (flags: HS_DT_AFFINE or 0; HS_DT_INVERSE is implied), applied to
 *           channel 0 and to the target: both back in metres, the bits hs_depth_target gives;
 *   use_logvar, total_mean, ranges [host], n_ranges   the metric rule, as hs_depth_metrics takes it (n_ranges <= 8);
 *   metric_partials [dev] f64[hs_expand_ln_head_blocks(tokens)][HS_DEPTH_NSUMS] scratch and metric_state [dev] f64[HS_DEPTH_NSUMS]
 *           (both or neither): the HS_DS_* sums of hs_depth_metrics over (metres, target in metres, channel 1) ADDED into the state:
 *           float64 per-lane sums, one record per workgroup, one ordered merge (a second, one-workgroup launch): no float
 *           atomics, the result depends on the grid only;
 *   preds   [dev] f32[n_out][4 tokens] or NULL: channel 0 in metres, channel 1 the raw log variance; 16-byte aligned;
 *   logvar_out [dev] f32[4 tokens] or NULL: channel 1 alone, written when preds is NULL (MeanSTDMedian's input); 16-byte aligned.
 * The log variance (use_logvar with a state, logvar_out) needs n_out == 2.  No head rows are needed for any of it (logits == NULL); y,
 * mean, rstd NULL is the validation form.  No host synchronisation, no allocation. */
int hs_expand_ln_head_depth_step_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec,
                                     const float* target, int kind, float huber_delta, int n_out, void* y, float* logits, float* mean,
                                     float* rstd, float* loss_partials, int flags, int transform, float shift, float scale, int use_logvar,
                                     double total_mean, const float* ranges, int n_ranges, double* metric_partials, double* metric_state,
                                     float* preds, float* logvar_out, int64_t tokens, int width, int children, int dtype, void* stream);
int hs_ln_head_depth_bwd(const void* y, const float* mean, const float* rstd, const float* target, int kind, float huber_delta,
                         const float* scale, int n_out, const void* wfold, const float* bvec, const void* afold, void* dy, void* dprime,
                         float* partials, int64_t rows, int width, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PatchMerging / PatchExpand / FinalPatchExpand_X4 as one operator call per module and direction (SURVEY 8b's proposed
 * hs_patch_merge_* / hs_patch_expand_*).  In nested HEALPix order the reference's data movement is a free view -- the four
 * strided slices + cat of PatchMerging (models_torch/swin_hp_transformer.py:385-390) are [B, N, C] -> [B, N/4, 4C], PatchExpand's
 * 'b n (p c) -> b (n p) c' (:427, :449) is [B, N, p c] -> [B, N p, c] -- so each module is a row LayerNorm and a bias-free
 * Linear.  These entry points chain the library's own kernels (hs_layernorm_*, hs_gemm_nt, hs_linear_wgrad) on the caller's
 * stream; bf16 only (HS_ERR_UNSUPPORTED otherwise: fp32 runs compose hs_layernorm_* with a library GEMM).
 *
 * hs_patch_merge_fwd   replaces PatchMerging.forward (:378-395):  out = LN_{4 dim}(x) W^T
 *   x [dev] bf16[rows, 4 dim] = the stage output [B, N, dim] viewed as [B N/4, 4 dim]; gamma, beta [dev] f32[4 dim];
 *   w [dev] bf16[dim_out, 4 dim] (nn.Linear layout; the reference has dim_out = 2 dim); normed [dev] bf16[rows, 4 dim],
 *   mean, rstd [dev] f32[rows]: saved for the backward; out [dev] bf16[rows, dim_out].
 *   Shapes (both directions): dim even, dim_out a multiple of 8, 4 dim <= 4096.
 * hs_patch_merge_bwd   its autograd: dx [dev] bf16[rows, 4 dim]; dw f32[dim_out, 4 dim], dgamma, dbeta f32[4 dim] overwritten
 *   (accumulate == 0) or added to (accumulate == 1: the callers' .grad buffers); w_t [dev] bf16[4 dim, dim_out] = the transposed
 *   weight; dnormed [dev] bf16[rows, 4 dim] scratch; workspace [dev] f32[hs_patch_merge_bwd_workspace(...)].
 * hs_patch_expand_fwd  replaces PatchExpand.forward (:418-430; children = 4, dim_exp = 2 dim) and FinalPatchExpand_X4.forward
 *   (:441-452; children = patch_size, dim_exp = patch_size dim):  out = LN_{dim_exp / children}( view(x W^T) )
 *   x [dev] bf16[rows, dim]; w [dev] bf16[dim_exp, dim]; gamma, beta f32[dim_exp / children]; expanded [dev] bf16[rows, dim_exp],
 *   mean, rstd [dev] f32[rows children]: saved; out [dev] bf16[rows children, dim_exp / children].
 *   Shapes (both directions): dim and dim_exp multiples of 8, children dividing dim_exp; the LayerNorm width dim_exp / children at
 *   most 4096 where it is a multiple of 8, at most 1024 otherwise.
 * hs_patch_expand_bwd  its autograd: w_t [dev] bf16[dim, dim_exp]; dexpanded [dev] bf16[rows, dim_exp] scratch; dx [dev]
 *   bf16[rows, dim]; dw f32[dim_exp, dim]; dgamma, dbeta f32[dim_exp / children]: overwritten or added to as for the merge;
 *   workspace as sized by the _workspace call.
 * accumulate (both backward operators) takes 0 and 1 ONLY.  With 0 every element of dw / dgamma / dbeta is written (the buffers may
 *   hold anything); with 1 the gradient is added once, and micro-batches may reuse one workspace (the calls are ordered by the
 *   stream).  dx is written either way.  HS_ACC_DEFER is not taken: the chained kernels take turns in one workspace (its size is the
 *   largest of theirs), so a deferred sum would find its partial records overwritten at the flush -- any other value returns
 *   HS_ERR_INVALID_ARG.
 * REFUSED MEANS UNTOUCHED: a forward and its backward accept the same shapes, and every argument, alignment and shape condition of
 *   every chained kernel is checked before the first launch; a call that returns HS_ERR_INVALID_ARG / _UNSUPPORTED / _MISALIGNED
 *   has launched nothing, written no output and queued nothing for hs_reduce_flush.
 * ---------------------------------------------------------------------------------------------- */
int hs_patch_merge_fwd(const void* x, const float* gamma, const float* beta, const void* w, void* normed, float* mean, float* rstd,
                       void* out, int64_t rows, int dim, int dim_out, int dtype, void* stream);
int64_t hs_patch_merge_bwd_workspace(int64_t rows, int dim, int dim_out);
int hs_patch_merge_bwd(const void* dout, const void* x, const void* normed, const float* gamma, const float* mean, const float* rstd,
                       const void* w_t, void* dnormed, void* dx, float* dw, float* dgamma, float* dbeta, float* workspace,
                       int accumulate, int64_t rows, int dim, int dim_out, int dtype, void* stream);
int hs_patch_expand_fwd(const void* x, const void* w, const float* gamma, const float* beta, void* expanded, float* mean, float* rstd,
                        void* out, int64_t rows, int dim, int dim_exp, int children, int dtype, void* stream);
int64_t hs_patch_expand_bwd_workspace(int64_t rows, int dim, int dim_exp, int children);
int hs_patch_expand_bwd(const void* dout, const void* x, const void* expanded, const float* gamma, const float* mean, const float* rstd,
                        const void* w_t, void* dexpanded, void* dx, float* dw, float* dgamma, float* dbeta, float* workspace,
                        int accumulate, int64_t rows, int dim, int dim_exp, int children, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flat Swin-UNet (models_torch/swin_transformer.py:SwinTransformerSys) in tiled Z order.
 * An Ht x Wt token grid is cut into T x T tiles laid out row-major; inside a tile the tokens follow a Morton order whose least
 * significant bit is the ROW bit.  With T = w * 2^(L-1) every window of every stage is w*w consecutive tokens and the
 * reference's PatchMerging concat order (0::2,0::2), (1::2,0::2), (0::2,1::2), (1::2,1::2) is four consecutive tokens.
 * ---------------------------------------------------------------------------------------------- */
/* z_of_rm [host] int32[Ht*Wt]: tiled-Z index of row-major token h*Wt + w; rm_of_z [host] its inverse.  Either may be NULL. */
int hs_flat_zorder(int Ht, int Wt, int T, int32_t* z_of_rm, int32_t* rm_of_z);
/* Shifted block of window side w and shift s (swin_transformer.py:312-347, :364-390) as a shifter table (see above), in tiled-Z
 * order: idx[j] = Z index of ((h+s) mod Ht, (w+s) mod Wt) for the cell (h, w) of Z position j (torch.roll by (-s, -s), then
 * window_partition); labels[j] = region of (h, w) in the img_mask slices (0,-w), (-w,-s), (-s,None) per dimension. */
int hs_build_flat_shift(int Ht, int Wt, int T, int w, int s, int32_t* idx, int32_t* inv, uint8_t* labels);
/* relative_position_index of the flat WindowAttention (swin_transformer.py:126-137) for a w x w window: row_major [host]
 * int64[w^4] as the reference's buffer, zorder [host] int64[w^4] with rows and columns in the in-window Morton order (what
 * the attention kernels read).  Either may be NULL. */
int hs_flat_rel_pos_index(int w, int64_t* row_major, int64_t* zorder);
/* The reference's dense attn_mask buffer [nW, w*w, w*w] in {0, -100}: windows row-major, positions row-major in a window.
 * out [host] float.  Only emitted by state_dict(); the kernels read labels. */
int hs_flat_attn_mask(int Ht, int Wt, int w, int s, float* out);

/* element types of the flat layout kernels, beside HS_F32 / HS_BF16 */
#define HS_U8 8
#define HS_I32 9
#define HS_I64 10
/* row layouts of the flat layout kernels */
#define HS_FLAT_PATCH_ROWS 0 /* row = token, column = (c, kh, kw) of the p x p patch (PatchEmbed's Conv2d as a Linear) */
#define HS_FLAT_PIXEL_ROWS 1 /* row = token * p^2 + kh * p + kw (FinalPatchExpand_X4's children), column = c */
/* [B, nch, H, W] image [dev] (HS_U8 / HS_F32 / HS_BF16; HS_I32 / HS_I64 too when out_dtype is HS_U8) -> token rows [dev] with
 * row pitch ld (elements) in out_dtype (HS_F32 / HS_BF16, or HS_U8 for labels: ids outside [0, 254] become 255).  Columns past
 * the valid ones are written as zeros.  H and W are multiples of p * T; T is a power of two. */
int hs_flat_img_to_rows(const void* img, int in_dtype, void* rows, int out_dtype, int batch, int nch, int H, int W, int p, int T,
                        int mode, int64_t ld, void* stream);
/* the inverse: token rows [dev] (HS_F32 / HS_BF16, padding columns ignored) -> [B, nch, H, W] image [dev] (HS_F32 / HS_BF16);
 * HS_U8 rows (class ids) go to a HS_U8 image bit for bit. */
int hs_flat_rows_to_img(const void* rows, int in_dtype, void* img, int out_dtype, int batch, int nch, int H, int W, int p, int T,
                        int mode, int64_t ld, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The flat data path (heal_swin_amd/flat_data.py, csrc/flat_data.hip): the reference's CenterCrop -> Resize -> Pad of a raw frame,
 * class mask or depth map (data/segmentation/flat_datasets.py:84-125, data/depth_estimation/flat_depth_datasets.py:69-147) and the
 * flat depth dataset's target chain, one pass per tensor, written EITHER as the NCHW result OR as the model's token rows.
 *   src       [dev] HS_U8 / HS_F32 [batch][nch][H0][W0], image b at b * src_stride_b (elements), the images themselves contiguous.
 *   row_idx   [dev] i32[2][H], col_idx [dev] i32[2][W]: per output row / column the two source taps (crop offset included), -1 in
 *             [0][.] for padding (value 0).  row_wgt [dev] f32[2][H], col_wgt [dev] f32[2][W]: the taps' weights (h0, h1), (w0, w1);
 *             value = h0*(w0*p00 + w1*p01) + h1*(w0*p10 + w1*p11) in fp32 without contraction, then for a HS_U8 source rounded half to
 *             even and cast.  Both weight tables NULL: nearest, tap [0][.] copied bit for bit.
 *   out       [dev] layout HS_FLAT_IMAGE: [batch][nch][H][W]; HS_FLAT_PATCH_ROWS / HS_FLAT_PIXEL_ROWS: the rows hs_flat_img_to_rows
 *             makes of that image (p, T, ld as there; ignored for HS_FLAT_IMAGE).  out_dtype HS_U8 / HS_F32 / HS_BF16 for a HS_U8
 *             source (the rounded uint8 value converted), HS_F32 for a HS_F32 source.
 *   flags, transform, shift, scale   HS_F32 sources: hs_depth_target's forward chain (HS_DT_1000_BKG, HS_DT_LOG / HS_DT_INV,
 *             HS_DT_AFFINE) applied to the resized, padded value; HS_DT_ZERO_BKG is not taken (the flat datasets keep zeros, so padding
 *             goes through the transform as 0).
 *   tile_h, tile_w   pixels of the output tile one workgroup owns (row layouts: S p square, S a power of two <= T); span_h, span_w:
 *             the most source rows / columns (last tap - first tap + 1) any such tile reads, from the caller's tables.  The tile's
 *             window is staged in hs_flat_resize_lds_bytes(...) bytes of LDS, at most 65536: HS_ERR_UNSUPPORTED otherwise (take a
 *             smaller tile).  Taps are clamped into the window and the source: wrong spans give wrong values, not wild accesses.
 * ---------------------------------------------------------------------------------------------- */
#define HS_FLAT_IMAGE 2 /* beside HS_FLAT_PATCH_ROWS / HS_FLAT_PIXEL_ROWS: the NCHW image itself */
int64_t hs_flat_resize_lds_bytes(int nch, int src_dtype, int tile_h, int tile_w, int span_h, int span_w);
int hs_flat_resize(const void* src, int src_dtype, int64_t src_stride_b, int batch, int nch, int H0, int W0, const int32_t* row_idx,
                   const float* row_wgt, const int32_t* col_idx, const float* col_wgt, void* out, int out_dtype, int H, int W, int layout,
                   int p, int T, int64_t ld, int tile_h, int tile_w, int span_h, int span_w, int flags, int transform, float shift,
                   float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HEALSWIN_H */
