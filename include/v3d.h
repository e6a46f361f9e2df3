/*
 * v3d.h - C ABI of libv3d_hip.so: the MI355X (gfx950) hot path of Video-3D-LLM's
 * position-aware video -> LLM forward path.
 *
 * The reference (zd11024/Video-3D-LLM) is pure Python: it has no FFI for this path.  The
 * boundary is therefore the set of PyTorch calls its hot path makes; each entry point below
 * names the reference site (file:line under the reference checkout) whose arithmetic it
 * replaces.  The host-side mirror (video-3d-llm_amd/llava/...) binds these with ctypes; see
 * INTEGRATION.md for the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all entry points are
 *     asynchronous with respect to the host, allocate nothing, keep no pointer after return
 *     and are re-entrant - with one exception: v3d_gemm keeps one 64 MiB device workspace per stream for the
 *     split-K tail of its 256-wide kernel (accumulator images of cut tiles), allocated by the first launch that
 *     takes that path and never during stream capture (V3D_GEMM_STREAMK=0 switches the path, and the allocation, off);
 *   - return value: 0 = ok, negative = error (V3D_E_*); the message for the calling thread is
 *     returned by v3d_last_error();
 *   - dtype codes: V3D_F32 / V3D_F16 / V3D_BF16.  16-bit tensors are raw IEEE half / bfloat16.
 *   - tensors are dense row-major unless a row stride (in elements) is passed explicitly.
 */
#ifndef V3D_H_
#define V3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V3D_ABI_VERSION 7   /* 2: *_rows decode entries, fp8 path, a7 / a3 device entries; 3: rope_kv_store, add_row, ...; 4: resize_bicubic, eos_update, embed_grad bounds; 6: sumsq, *_rows entries take 1..32 rows; 7: attention_shared_prefix; ground_scores_rows, add_rows and the v3d_beam_* entries were ADDED under 7 (no entry changed); so were the v3d_sample_* entries, and v3d_coord_points_voxel, v3d_sin3d_table_points_layout, v3d_sin3d_table_build_points, v3d_sin3d_pe_points and v3d_visual_tokens_points; and v3d_pe_mlp_hidden, v3d_visual_tokens_rows, v3d_visual_tokens_rows_grad, v3d_pe_mlp_wgrad_workspace_bytes and v3d_pe_mlp_wgrad; and v3d_lora_down, v3d_lora_wgrad_chunk, v3d_lora_wgrad_workspace_bytes and v3d_lora_wgrad */

enum { V3D_F32 = 0, V3D_F16 = 1, V3D_BF16 = 2 };
enum { V3D_U8_HWC = 16 };   /* v3d_resize_bicubic_u8 only: 8-bit interleaved output, no normalisation */

enum {
  V3D_OK = 0,
  V3D_E_INVALID = -1,   /* bad argument (null pointer, shape or alignment the kernel cannot take) */
  V3D_E_LAUNCH = -2,    /* HIP reported a launch/runtime error */
  V3D_E_UNSUPPORTED = -3
};

int v3d_abi_version(void);
const char* v3d_last_error(void);

/* ------------------------------------------------------------------ geometry (K1-K4) ---- */

/* K1  llava/video_utils.py:38-68 `unproject`.
 * depth_mm [V,H,W] f32 millimetres, intrinsics/poses [V,4,4] f32 -> world [V,H,W,3] f32. */
int v3d_unproject_f32(const float* depth_mm, const float* intrinsics, const float* poses,
                      float* world, int V, int H, int W, void* stream);

/* K1+K2  `unproject` evaluated only at the pixels that survive the nearest-neighbour resize
 * (cv2.resize INTER_NEAREST to (int(W*crop/H), crop)) and centre crop of
 * llava/video_utils.py:296-308.  depth [V,H,W] uint16 PNG values (the reference converts
 * u16 -> int32 -> f32, video_utils.py:217,230).  out [V,crop,crop,3] in out_dtype
 * (f32 = the tensor VideoProcessor returns; f16/bf16 = after the eval driver's
 * `.half()` / model-dtype cast, llava/eval/model_scanqa.py:163-165). */
int v3d_unproject_sampled_u16(const uint16_t* depth, const float* intrinsics, const float* poses,
                              void* out, int out_dtype, int V, int H, int W, int crop, void* stream);

/* VideoProcessor.preprocess, strategy "resize" (video_utils.py:293-296): the back-projection at the pixels cv2.resize(coords, (size, size),
 * INTER_NEAREST) keeps, both axes scaled independently, no crop: out [V,size,size,3].  (Index rule restated as for the centre-crop form:
 * parity unpinned, cv2 is absent.) */
int v3d_unproject_resized_u16(const uint16_t* depth, const float* intrinsics, const float* poses, void* out, int out_dtype, int V, int H,
                              int W, int size, void* stream);

/* calculate_world_coords(do_normalize=True) (video_utils.py:232-236; the "norm" frame-sampling strategies): xyz [n_points, 3] clamped
 * in place to [lo, hi] per axis (host float[3] each). */
int v3d_clamp_xyz(void* xyz, int64_t n_points, const float* lo_host, const float* hi_host, int dtype, void* stream);

/* llava/video_utils.py:268-273 `boundry`: [x_min, x_max, y_min, y_max, z_min, z_max] of `unproject` over ALL V*H*W pixels (taken
 * before the resize and crop), computed without materialising the full-resolution tensor: same per-pixel arithmetic as
 * v3d_unproject_f32 on the u16 depth, reduced on the fly.  bounds: 6 floats (device).  workspace: device scratch of at
 * least v3d_unproject_bounds_workspace_bytes(V) bytes. */
int64_t v3d_unproject_bounds_workspace_bytes(int V);
int v3d_unproject_bounds_u16(const uint16_t* depth, const float* intrinsics, const float* poses, int V, int H, int W,
                             float* bounds, void* workspace, int64_t workspace_bytes, void* stream);

/* K3+K4  llava/model/llava_arch.py:213-223 `average_coordinate_in_patch` and :259-272
 * `discrete_coords`.  coords [V,S,S,3] (dtype), the last S - n*patch rows/cols are dropped
 * (n = (S-6)/patch when S==384, patch==27 -> n = 14).  The 27x27 mean is accumulated in f32
 * in the reference's own (row, column) order so that voxel ids are bit-exact.
 * Outputs (any may be NULL): avg [V,n,n,3] dtype; vox [V,n,n,3] dtype (integer-valued floats,
 * what the reference returns); ids [V,n,n,3] int32.
 * min_xyz_host/max_xyz_host: 3 floats each on the HOST (config.min_xyz_range / max_xyz_range). */
int v3d_coord_pool_voxel(const void* coords, int dtype, int V, int S, int patch,
                         const float* min_xyz_host, const float* max_xyz_host, float voxel_size,
                         void* avg, void* vox, int32_t* ids, void* stream);

/* K4 alone on arbitrary points: xyz [N,3] dtype -> vox [N,3] dtype and/or ids [N,3] int32
 * (box centres / box_input path, llava_arch.py:416-420). */
int v3d_discrete_coords(const void* xyz, int dtype, int64_t N, const float* min_xyz_host,
                        const float* max_xyz_host, float voxel_size, void* vox, int32_t* ids,
                        void* stream);

/* ------------------------------------------------------------------ 3-D sinusoid (K5) --- */

/* Number of elements of one row of the shifted 16-byte-aligned PE table for `embedding_size`
 * channels of `dtype` (see v3d_sin3d_table_build). */
int64_t v3d_sin3d_table_row_elems(int embedding_size, int dtype);

/* llava/model/position_encoding.py:17-49 evaluated for every integer coordinate 0..n_ids-1.
 * dim_t [num_feats = embedding_size/3] f32 is supplied by the caller (the reference computes
 * `temperature ** (2*(i//2)/num_feats)` with torch's pow, :24-25; pow is not bit-reproducible
 * across libraries so it stays on the caller's side of the boundary).
 * table [3][n_ids][row_elems] dtype: axis a's copy is shifted by (a*num_feats) % (16/sizeof)
 * elements so that the fused kernel reads whole 16-byte vectors; padding is zero.
 * table_f32 (nullable) [n_ids][num_feats] f32: the unshifted f32 values. */
int v3d_sin3d_table_build(const float* dim_t, int embedding_size, int n_ids, int dtype,
                          void* table, float* table_f32, void* stream);

/* PositionEmbeddingSine3D.forward for arbitrary (also non-integer) coordinates:
 * xyz [N,3] dtype -> out [N,embedding_size] dtype; f32 math, output cast to dtype (:46-47). */
int v3d_sin3d_pe(const void* xyz, int dtype, int64_t N, const float* dim_t, int embedding_size,
                 void* out, void* stream);

/* ------------------------------------------------------------------ fusion (K5-K8) ------ */

/* The north-star kernel.  One pass over the projector output:
 *   K7  get_2dPool bilinear side x side -> n x n            llava_arch.py:191-210   (flag POOL)
 *   K5+K6  + PE(voxel ids) from the table                    llava_arch.py:506-517   (flag PE)
 *   K8  add_token_per_grid: `newline` after each row of n    llava_arch.py:307-328   (flag NEWLINE)
 * feat  [V, side*side, C] if POOL else [V, n*n, C]           (dtype)
 * ids   [V, n*n, 3] int32 voxel ids (PE only)
 * table from v3d_sin3d_table_build for (C, dtype), n_ids rows per axis (PE only)
 * newline [C] dtype (NEWLINE only)
 * out   rows of C elements, row stride out_stride elements: V*n*(n+1) rows if NEWLINE else V*n*n.
 * Rounding follows the reference: pooled value rounded to dtype, then the add rounded to dtype. */
enum { V3D_VT_POOL = 1, V3D_VT_PE = 2, V3D_VT_NEWLINE = 4 };
int v3d_visual_tokens(const void* feat, const int32_t* ids, const void* table, int n_ids,
                      const void* newline, void* out, int64_t out_stride, int dtype, int V, int side,
                      int n, int C, int flags, void* stream);

/* ------------------------------------------------- the other position encodings (P points) ---- */

/* llava_arch.py:225-257 `sample_n_points` / `minmax_coordinate_in_patch` followed by :259-272 `discrete_coords`: the
 * world_position_embedding_type variants other than `avg` (which stays on v3d_coord_pool_voxel).
 * coords [V,S,S,3] (dtype); S must be 384 and patch 27 (the reference hard-codes a 14 x 27 grid, :245), n = 14.
 *   SAMPLE9  pixel (27*py + {4,13,22}, 27*px + {4,13,22}) of every patch, point index 3*ri + ci      P = 9
 *   SAMPLE5  points 0, 2, 4, 6, 8 of those                                                            P = 5
 *   SAMPLE1  point 4 of those                                                                         P = 1
 *   MINMAX   point 0 the per-axis minimum over the 27x27 patch, point 1 the maximum; a NaN in the patch gives NaN  P = 2
 * Outputs (any may be NULL), all [V,n,n,P,3]: pts dtype (exact copies of input values); vox dtype (integer-valued,
 * what `discrete_coords` returns); ids int32.  The sample modes read P pixels per patch, never the frame; MINMAX
 * reads the first 378 rows once (coords 16-byte aligned).  min_xyz_host / max_xyz_host: 3 floats each on the HOST. */
enum { V3D_PTS_SAMPLE9 = 0, V3D_PTS_SAMPLE5 = 1, V3D_PTS_SAMPLE1 = 2, V3D_PTS_MINMAX = 3 };
int v3d_coord_points_voxel(const void* coords, int dtype, int V, int S, int patch, int mode,
                           const float* min_xyz_host, const float* max_xyz_host, float voxel_size,
                           void* pts, void* vox, int32_t* ids, void* stream);

/* Layout of the PE table for PositionEmbeddingSine3D(embedding_size, n_points) (position_encoding.py:17-49):
 * num_feats = embedding_size / (3*n_points) must be at least 16/sizeof(dtype).  Segment q (point q/3, axis q%3) of a
 * token row starts (q*num_feats) % (16/sizeof) elements past a 16-byte boundary; the table keeps one copy of the
 * [n_ids, num_feats] values per DISTINCT such shift.  Returns the number of copies (1..16/sizeof), or a negative
 * error; writes the elements of one row to *row_elems_host and copy c's shift to shifts_host[c] (host pointers,
 * either may be NULL; shifts_host holds up to 8 entries). */
int v3d_sin3d_table_points_layout(int embedding_size, int n_points, int dtype, int64_t* row_elems_host,
                                  int32_t* shifts_host);

/* The table itself: table [n_copies][n_ids][row_elems] dtype, copy c holding T(PE value) of id at elements
 * shift_c .. shift_c + num_feats - 1 of its row and zero bits elsewhere.  dim_t [num_feats] f32 from the caller, as for
 * v3d_sin3d_table_build. */
int v3d_sin3d_table_build_points(const float* dim_t, int embedding_size, int n_points, int n_ids, int dtype,
                                 void* table, void* stream);

/* PositionEmbeddingSine3D(embedding_size, n_points).forward for arbitrary coordinates: xyz [N,n_points,3] dtype ->
 * out [N,embedding_size] dtype.  Channel c < 3*n_points*num_feats: q = c / num_feats, j = c % num_feats,
 * sin (j even) or cos (j odd) of xyz[q] / dim_t[j]; f32 IEEE division, correctly rounded trig, one cast to dtype; the
 * remaining channels are 0.  Box centres and object centres are encoded with the centre repeated n_points times
 * (llava_arch.py:409-413). */
int v3d_sin3d_pe_points(const void* xyz, int dtype, int64_t N, int n_points, const float* dim_t,
                        int embedding_size, void* out, void* stream);

/* v3d_visual_tokens with n_points points per token (flags POOL, NEWLINE as there; PE is required).  The PE operand is
 *   ids [V, n*n, n_points, 3] int32 + table from v3d_sin3d_table_build_points for (C, n_points, dtype)   (default), or
 *   pts [V, n*n, n_points, 3] dtype + dim_t [C/(3*n_points)] f32, trig evaluated per channel (flag CONTINUOUS: a type
 *   without `discrete`, llava_arch.py:509-512; serves `avg-sin3d` with n_points = 1 too).
 * The unused pair may be NULL.  Same rounding points as v3d_visual_tokens; with n_points = 1 and ids the output equals
 * v3d_visual_tokens bit for bit, and with integer-valued pts the CONTINUOUS form equals the table form. */
enum { V3D_VT_CONTINUOUS = 8 };
int v3d_visual_tokens_points(const void* feat, const int32_t* ids, const void* pts, const void* table, int n_ids,
                             const float* dim_t, int n_points, const void* newline, void* out, int64_t out_stride,
                             int dtype, int V, int side, int n, int C, int flags, void* stream);

/* Added under ABI 7 (no entry changed).  PositionEmbeddingMLP (position_encoding.py:52-84; selected by an `mlp`
 * world_position_embedding_type, llava_arch.py:60-61): Linear(3, 512) -> LayerNorm(512, eps) -> ReLU -> Linear(512, E).
 * The rule is DESIGN section 2, "The MLP position encoding, stated once".  16-bit dtypes only.
 *
 * The first three stages: x [N,3], w0 [hidden,3], b0 / ln_w / ln_b [hidden], all dtype ->
 *     z = T(x . w0^T + b0)                        (three fused multiply-adds per element, one rounding)
 *     h = relu(T((z - mean) * rstd * ln_w + ln_b))  (row statistics of the ROUNDED z in f32)
 * h [N,hidden] dtype; z [N,hidden] dtype is optional (NULL: not stored) - training keeps it, the tests isolate the stages
 * with it.  hidden must be 512 (the reference's only width; one wave per row, 8 elements per lane); any N >= 1; rows are
 * independent (a NaN coordinate gives a NaN row and nothing else).  The last stage is v3d_gemm(h, w3, V3D_EPI_BIAS). */
int v3d_pe_mlp_hidden(const void* x, const void* w0, const void* b0, const void* ln_w, const void* ln_b, float eps,
                      int64_t N, int hidden, int dtype, void* z, void* h, void* stream);

/* v3d_visual_tokens with the PE read from rows: pe [V*n*n, C] dtype, row stride pe_stride (a multiple of 8), row
 * (v*n + oh)*n + ow added to output token (v, oh, ow).  Flags POOL and NEWLINE as there (PE is implied); the same rounding
 * points: token = T(T(pooled) + pe).  feat is read once and out written once; the PE rows are the extra traffic. */
int v3d_visual_tokens_rows(const void* feat, const void* pe, int64_t pe_stride, const void* newline, void* out,
                           int64_t out_stride, int dtype, int V, int side, int n, int C, int flags, void* stream);

/* Backward of v3d_visual_tokens_rows: dfeat and dnewline exactly as v3d_visual_tokens_grad gives them (same kernels), plus
 * dpe [V*n*n, C] dtype (row stride dpe_stride): the gradient rows of the tokens without the newline rows - the add passes
 * the gradient through, and the two linears below it take it as a plain matrix. */
int v3d_visual_tokens_rows_grad(const void* dout, int64_t dout_stride, void* dfeat, float* dnewline, void* dpe,
                                int64_t dpe_stride, int dtype, int V, int side, int n, int C, int flags, void* stream);

/* Weight gradient of the first Linear: dw0[j, a] = sum over rows r of dz[r, j] * x[r, a]; dz [rows, hidden] dtype (row
 * stride lddz), x [rows, 3] dtype, dw0 [hidden, 3] in out_dtype.  f32, fixed order, no atomics (32-row partials in row order,
 * then the partials as v3d_colsum sums them): run-to-run identical.  hidden must be 512.
 * workspace: v3d_pe_mlp_wgrad_workspace_bytes(rows, hidden) bytes. */
int64_t v3d_pe_mlp_wgrad_workspace_bytes(int64_t rows, int hidden);
int v3d_pe_mlp_wgrad(const void* dz, int64_t lddz, const void* x, int64_t rows, int hidden, int dtype, float* workspace,
                     void* dw0, int out_dtype, void* stream);

/* K9  embed_tokens gather for the text segments (llava_arch.py:693): out[i,:] = table[ids[i],:]. */
int v3d_embed_gather(const void* table, int64_t vocab, int C, const int64_t* ids, int64_t n,
                     void* out, int64_t out_stride, int dtype, void* stream);

/* ------------------------------------------------------------------ dense linears ------- */

/* K10-K12, K15, K17  every nn.Linear on the path (SigLIP q/k/v/out/fc1/fc2 and patch embedding,
 * siglip_encoder.py:156-174,197-265; mlp2x_gelu projector, multimodal_projector/builder.py:41-48;
 * Qwen2 q/k/v/o and gate/up/down, modeling_qwen2.py:177-189,237-240,322):
 *     out[M, N'] = epilogue( A[M,K] . W[N,K]^T ),   16-bit operands, f32 MFMA accumulation.
 * A row stride lda, W row stride ldw (elements).  N % 128 == 0 and K % 64 == 0 (pad weights with
 * zero rows / columns once at load); M is arbitrary (M <= 8 takes a weight-streaming path for decode).
 * Epilogues (rounding points as torch: linear output rounded to dtype, then each further op):
 *   NONE            out = acc
 *   BIAS            out = acc + bias[n]
 *   BIAS_GELU_ERF   out = gelu(acc + bias)            nn.GELU()            (projector)
 *   BIAS_GELU_TANH  out = gelu_tanh(acc + bias)       gelu_pytorch_tanh    (SigLIP fc1)
 *   BIAS_RES        out = res[m or m % res_mod, n] + (acc + bias)          (SigLIP out_proj/fc2, patch-embed + pos-emb)
 *   RES             out = res[m, n] + acc                                  (Qwen2 o_proj / down_proj)
 *   SWIGLU          out[m, j] = silu(gate_j) * up_j, N' = N/2; W rows are tile-interleaved: rows
 *                   [128t, 128t+64) = gate rows [64t, 64t+64), rows [128t+64, 128t+128) = the up rows.
 * Summation order: every kernel sums k in ascending order in one run per output - except tiles the split-K tail cuts
 * (M x N x K shapes whose 256 x 256 tiles leave the last round of the chip under half full, e.g. 6794 x 3584 x 18944),
 * which are the f32 sum of 2..4 runs: such an output may differ from the one-run result by one rounding of the
 * 16-bit value.  v3d_gemm_plan_host reports the plan; V3D_GEMM_STREAMK=0 keeps every output on one run. */
enum {
  V3D_EPI_NONE = 0, V3D_EPI_BIAS = 1, V3D_EPI_BIAS_GELU_ERF = 2, V3D_EPI_BIAS_GELU_TANH = 3,
  V3D_EPI_BIAS_RES = 4, V3D_EPI_RES = 5, V3D_EPI_SWIGLU = 6,
  V3D_EPI_BIAS_RELU = 7   /* out = relu(acc + bias)   grounding head, llava_qwen.py:93-104 */
};
int v3d_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, const void* res,
             int64_t ldr, int res_mod, void* out, int64_t ldo, int M, int N, int K, int dtype, int epilogue,
             void* stream);
/* The same product with a layout flag per operand: out[M, N] = epilogue(op(A) . op(B)).
 *   kmajor = 0   element (row r, k) at ptr[r * ld + k] (K-contiguous: v3d_gemm's layout), ld >= K;
 *   kmajor = 1   element (row r, k) at ptr[k * ld + r]: the stored matrix is [K, rows], contiguous along the output dimension,
 *                ld >= rows (M for A, N for B).
 * (0, 1) is dx = dy . W on an nn.Linear weight as stored, (1, 1) dW = dy^T . x on dy and x as stored - the two products of a
 * linear's backward without a transposed copy (v3d/train.py: linear_backward under V3D_TRAIN_GEMM_LAYOUTS=1).  (0, 0) IS v3d_gemm
 * (forwarded unchanged).  With a k-major operand: 16-bit MFMA tile kernels only (128 x 128 x 64, or 256 x 256 x 64 where N % 256 == 0
 * and the cost model prefers it; V3D_GEMM_LAYOUT_TILE=128 / 256 forces one, read per call), no skinny path, no split-K tail;
 * epilogues NONE and RES only (`bias` is not read), every other one is refused with V3D_E_INVALID;
 * N % 128 == 0; every ld a multiple of 8; pointers 16-byte aligned; a k-major A needs M % 8 == 0;
 * K % 64 == 0 unless BOTH operands are k-major - then K is a row count and any K >= 1 is taken (the k-rows past K of the last
 * K-step are read from a zero-filled line, never from the operands); an operand spans fewer than 2^31 elements.
 * Summation order: k ascending in one run per output; rounding points as v3d_gemm.  All checks run before any device call. */
int v3d_gemm_layout(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor,
                    const void* bias, const void* res, int64_t ldr, int res_mod, void* out, int64_t ldo,
                    int M, int N, int K, int dtype, int epilogue, void* stream);

/* FP8 (OCP e4m3) variant of the LLM linears - BASELINE configs[3]; not part of the reference (tolerance is
 * re-stated in tests/test_gpu_fp8.py).  y[m,n] = sa[m] * sw[n] * sum_k qa[m,k] qw[n,k] with per-row scales.
 * v3d_quantize_fp8_rows: x [rows, cols] (f16/bf16) -> q [rows, cols] e4m3 bytes (row stride ldq) + scale[rows] f32,
 *   scale = amax|row| / 448 in f32, floored at the smallest normal f32 (2^-126) so that 1 / scale stays finite for rows of
 *   subnormal size; an all-zero row gets scale 1 and zero bytes.  q = e4m3(x * (1 / scale)), round to nearest even.  Used for
 *   activations per call and for weights once at load.
 * v3d_gemm_fp8: A [M,K] e4m3 (lda bytes), W [N,K] e4m3; N % 256 == 0, K % 128 == 0; epilogues NONE / BIAS / RES /
 *   SWIGLU (same codes and row interleave as v3d_gemm); output in out_dtype (f16 / bf16). */
int v3d_quantize_fp8_rows(const void* x, int64_t ldx, int64_t rows, int cols, int dtype, void* q, int64_t ldq,
                          float* scale, void* stream);
int v3d_gemm_fp8(const void* A, int64_t lda, const float* scale_a, const void* W, int64_t ldw, const float* scale_w,
                 const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int M, int N, int K,
                 int out_dtype, int epilogue, void* stream);
/* v3d_rmsnorm fused with v3d_quantize_fp8_rows of its output (the 16-bit normalised row is formed and rounded exactly as
 * v3d_rmsnorm does, but never stored): q [rows, cols] e4m3 + scale[rows].  Bit-identical to the two calls in sequence
 * (rows > 4; v3d_rmsnorm's decode-order kernel for <= 4 rows sums in another order).  cols <= 4096. */
int v3d_rmsnorm_quantize_fp8(const void* x, int64_t ldx, const void* weight, float eps, int64_t rows, int cols, int dtype,
                             void* q, int64_t ldq, float* scale, void* stream);

/* MXFP4 (OCP MX v1.0) weights for the LLM linears; not part of the reference (contract and tolerances are stated in
 * tests/test_gpu_fp4.py, the format is restated on the host in tests/mxfp4_check.py).  A weight matrix W [N, K]
 * (K % 128 == 0) is the pair
 *   q [N, K/2] bytes: two e2m1 codes per byte, the even k in the low nibble; code = sign(1) | exp(2) | mant(1), magnitudes
 *                     {0, 0.5, 1, 1.5, 2, 3, 4, 6};
 *   e [N, K/32] bytes: one E8M0 exponent per 32 consecutive k of a row, value 2^(e - 127); 0xFF is never written.
 * v3d_quantize_mxfp4_rows: w [rows, cols] (f16/bf16, finite) -> (q, e), row strides ldq / lde in bytes.  Per block:
 *   e = clamp(floor(log2(amax)) - 2 + 127, 0, 254), an all-zero block gets e = 127; codes = w * 2^(127 - e) rounded to the
 *   nearest e2m1 value, ties to the even code, saturating at +-6; a zero magnitude carries no sign.
 * v3d_gemm_mxfp4 (prefill, W4A8): y[m,n] = scale_a[m] * sum_k A[m,k] * deq(W)[n,k], A [M,K] e4m3 (lda bytes) + scale_a as
 *   v3d_quantize_fp8_rows / v3d_rmsnorm_quantize_fp8 write them; f32 accumulation; N % 256 == 0, K % 128 == 0, any M >= 1;
 *   epilogues NONE / BIAS / RES / SWIGLU with the codes, rounding order and row interleave of v3d_gemm_fp8. */
int v3d_quantize_mxfp4_rows(const void* w, int64_t ldw, int64_t rows, int cols, int dtype, void* q, int64_t ldq, void* e,
                            int64_t lde, void* stream);
int v3d_gemm_mxfp4(const void* A, int64_t lda, const float* scale_a, const void* Wq, int64_t ldw, const void* We, int64_t lde,
                   const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int M, int N, int K, int out_dtype,
                   int epilogue, void* stream);

/* ------------------------------------------------------------------ norms / rotary ------ */

/* K13  Qwen2RMSNorm, modeling_qwen2.py:85-90: out = weight * T(x * rsqrt(mean(x^2) + eps)), f32 inside. */
int v3d_rmsnorm(const void* x, int64_t ldx, const void* weight, void* out, int64_t ldo, int64_t rows,
                int cols, float eps, int dtype, void* stream);

/* nn.LayerNorm of the SigLIP encoder layers, siglip_encoder.py:272-274,292,300 (f32 statistics). */
int v3d_layernorm(const void* x, int64_t ldx, const void* weight, const void* bias, void* out,
                  int64_t ldo, int64_t rows, int cols, float eps, int dtype, void* stream);

/* K14  Qwen2RotaryEmbedding.forward, modeling_qwen2.py:106-129, for positions 0..n_pos-1:
 * cos/sin tables [n_pos, head_dim/2] in dtype.  inv_freq [head_dim/2] f32 comes from the caller
 * (the reference evaluates 1/(base**(arange/dim)) with torch on the host, :100). */
int v3d_rope_table_build(const float* inv_freq, int head_dim, int n_pos, int dtype, void* cos_table,
                         void* sin_table, void* stream);

/* apply_rotary_pos_emb, modeling_qwen2.py:141-173, in place on n_heads heads of head_dim laid out
 * contiguously from x in every token row (row stride ldx).  Token t uses positions[t] if positions
 * is non-NULL, else pos0 + t.  (The three M-RoPE position rows are identical on this path, :1003.) */
int v3d_rope_apply(void* x, int64_t ldx, int64_t tokens, int n_heads, int head_dim,
                   const void* cos_table, const void* sin_table, int n_pos, const int32_t* positions,
                   int pos0, int dtype, void* stream);

/* Prefill form of K14 + the KV-cache append in one pass (modeling_qwen2.py:141-173, then DynamicCache.update as called at
 * :283-285): rotary in place on the n_q query heads of every QKV row; the rotated key heads and the value heads of token t
 * go to cache + r*ldc, r = dst_rows[t] (device int64 array) or row0 + t, laid out [k heads | v heads].  The k/v columns of
 * the QKV buffer itself are left unrotated.  Token t uses positions[t] (device int32) or pos0 + t.  dst_rows lets several
 * questions of one scene, prefilled together, append to their own caches inside one allocation. */
int v3d_rope_kv_store(void* qkv, int64_t ldx, int64_t tokens, int n_q_heads, int n_kv_heads, int head_dim,
                      const void* cos_table, const void* sin_table, int n_pos, const int32_t* positions, int pos0,
                      void* cache, int64_t ldc, const int64_t* dst_rows, int64_t row0, int dtype, void* stream);

/* llava_arch.py:697-700: x[rows[i], 0:C] += add[0:C] (the box-centre PE on the <coord> token rows of inputs_embeds);
 * rows: device int64 [n_rows]; 16-bit dtypes; the sum is rounded once to dtype. */
int v3d_add_row(void* x, int64_t ldx, const int64_t* rows, int n_rows, int C, const void* add, int dtype, void* stream);

/* The same add with one source row per destination row: x[rows[i], 0:C] += add[src[i], 0:C] (add: [*, lda]) - the box-centre PEs of a
 * batch of Scan2Cap questions on their <coord> rows in one launch.  rows, src: device int64 [n_rows].  rows must be DISTINCT (each
 * destination row belongs to one workgroup; a repeated row is a race); src may repeat (two <coord> tokens of one question take the
 * same PE).  Any C > 0, ldx, lda >= C: 16-byte accesses where ldx % 8 == lda % 8 == 0 and both bases are 16-byte aligned, the
 * columns past 8 floor(C / 8) (or all of them) one by one.  With every src equal it is v3d_add_row bit for bit. */
int v3d_add_rows(void* x, int64_t ldx, const int64_t* rows, const int64_t* src, int n_rows, int C, const void* add, int64_t lda,
                 int dtype, void* stream);

/* ------------------------------------------------------------------ attention ----------- */

/* K16 / K11  softmax(Q K^T * scale [+ causal mask]) V without materialising the scores.
 * Prefill: Qwen2 causal GQA (spec: eager Qwen2Attention, modeling_qwen2.py:289-311; runtime:
 * flash-attn-2 :567-574) with D = 128; SigLIP attention (siglip_encoder.py:213-239) non-causal with
 * D = 96 = the kernel's tile width for head dim 72: d_out = 72 is the number of valid dims - columns >= d_out of q are
 * treated as zero and only d_out columns of o are written, so heads may be packed at their true stride (hsq = hsk = 72:
 * the 24 extra columns a tile row covers then belong to the next head or to row padding; they must be readable).
 * Element (b, token s, head h, dim d) of q is at q + b*bsq + s*ldq + h*hsq + d (likewise k, v with
 * bsk/ldk|ldv/hsk and o with bso/ldo/hso); kv head = h / (Hq/Hkv).  With causal != 0 query i sits at
 * key position q_pos0 + i (q_pos0 = number of cached tokens).  Sq <= 8 with B == 1 takes the
 * cache-streaming decode path. */
int v3d_attention(const void* q, const void* k, const void* v, void* o, int dtype, int B, int Sq, int Sk,
                  int Hq, int Hkv, int D, int d_out, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                  int64_t bsq, int64_t bsk, int64_t bso, int hsq, int hsk, int hso, int causal, int q_pos0,
                  float scale, void* stream);

/* r04 (scene reuse): v3d_attention (causal, D = 128) for the question rows of B questions about ONE prefilled scene -
 * the reference recomputes the scene for every question (model_scanqa.py:130-185; the shared prompt: :46-60).  Key tiles below
 * shared_len (a multiple of 64, <= q_pos0) are read from the scene's cache k_shared / v_shared (ldk / ldv / hsk as k / v, no batch
 * stride); keys from shared_len on from k / v + b*bsk (each question's own cache, rows at their absolute positions: rows below
 * shared_len of those caches are never touched).  A workgroup's query slots hold the rows of all query heads of a kv head.  Every
 * output bit equals v3d_attention's on B full copies. */
int v3d_attention_shared_prefix(const void* q, const void* k, const void* v, const void* k_shared, const void* v_shared,
                                int shared_len, void* o, int dtype, int B, int Sq, int Sk, int Hq, int Hkv, int64_t ldq,
                                int64_t ldk, int64_t ldv, int64_t ldo, int64_t bsq, int64_t bsk, int64_t bso, int hsq, int hsk,
                                int hso, int q_pos0, float scale, void* stream);

/* Decode step of K16 (one new query row against the K/V cache, modeling_qwen2.py:282-311 with a
 * DynamicCache): split-KV so the cache is streamed once by the whole chip.  q [Hq*128] (head stride hsq),
 * caches [Sk, ...] with row strides ldk/ldv and kv-head stride hsk, o [Hq*128] (head stride hso).
 * workspace: device scratch of at least v3d_attention_decode_workspace_bytes(Hq, 1024/Hkv) bytes. */
int64_t v3d_attention_decode_workspace_bytes(int Hq, int max_splits);
int v3d_attention_decode(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int Sk,
                         int Hq, int Hkv, int64_t ldk, int64_t ldv, int hsq, int hsk, int hso, float scale,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* The same for M = 1..32 (r04; was 16) scenes decoding together in ONE launch pair (the single-scene kernels are latency-bound, not
 * bandwidth-bound): query rows q + m*q_stride, outputs o + m*o_stride (elements), per-scene cache pointers and lengths
 * in HOST arrays of M entries; workspace >= M * v3d_attention_decode_workspace_bytes(Hq, 1024/Hkv).  Scene m's output
 * is bit-identical to v3d_attention_decode on it alone, whatever the other scenes' lengths: every scene partitions its keys
 * by its own length (256 keys per split), the launch only adds empty splits for the shorter ones. */
int v3d_attention_decode_rows(const void* q, int64_t q_stride, int M, const void* const* k_caches,
                              const void* const* v_caches, const int* Sk, void* o, int64_t o_stride, int dtype, int Hq,
                              int Hkv, int64_t ldk, int64_t ldv, int hsq, int hsk, int hso, float scale, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* Scene-level reuse: the M rows are questions about ONE scene whose caches all start with the same prefix_len rows
 * (the scene's [system | user | <image>] K/V, broadcast into each question's cache).  Keys < prefix_len are read from k_prefix /
 * v_prefix (same strides as the caches; any one of the copies) for every question, so the chip streams the prefix once per step
 * instead of M times; rows >= prefix_len come from the question's own cache.  Outputs are bit-identical to
 * v3d_attention_decode_rows on the same caches. */
int v3d_attention_decode_rows_prefix(const void* q, int64_t q_stride, int M, const void* k_prefix, const void* v_prefix,
                                     int prefix_len, const void* const* k_caches, const void* const* v_caches, const int* Sk,
                                     void* o, int64_t o_stride, int dtype, int Hq, int Hkv, int64_t ldk, int64_t ldv, int hsq,
                                     int hsk, int hso, float scale, void* workspace, int64_t workspace_bytes, void* stream);

/* Decode-step linear (one activation row; K15/K17/K18 at q_len == 1): y = epilogue(W . f(x)), W [N,K] row
 * stride ldw.  norm_weight != NULL fuses Qwen2RMSNorm (modeling_qwen2.py:85-90) in front: f(x) = w * T(x*rstd).
 * epilogue: 0 NONE, 1 BIAS (y += bias), 2 RES (y = res + T(y)), 3 SWIGLU (tile-interleaved gate|up rows as
 * v3d_gemm's SWIGLU; N' = N/2).  Weights are streamed once with non-temporal loads. */
enum { V3D_DEC_NONE = 0, V3D_DEC_BIAS = 1, V3D_DEC_RES = 2, V3D_DEC_SWIGLU = 3 };
int v3d_linear_decode(const void* x, const void* norm_weight, float eps, const void* W, int64_t ldw,
                      const void* bias, const void* res, void* out, int N, int K, int dtype, int epilogue,
                      void* stream);
/* The same linear for M activation rows at once (M scenes decoding together share one pass over the weights; the
 * step is HBM-bound on them).  x [M, K] row stride ldx, res [M, N] row stride ldr, out [M, N'] row stride ldo.
 * M = 1 is v3d_linear_decode.  M = 2..32 (r04; two 16-row blocks per weight fragment above 16; no fused norm, K % 128 == 0, N % 16 == 0): the weights feed the matrix cores
 * (v_mfma_f32_16x16x32, activation rows as the B operand), so the cost does not grow with M and a row's result does not
 * depend on the other rows or on M; against the one-row form it differs by the f32 summation order only.  Other shapes
 * (fused norm, odd sizes): VALU form, M = 1..4, each row bit-identical to v3d_linear_decode on it. */
int v3d_linear_decode_rows(const void* x, int64_t ldx, int M, const void* norm_weight, float eps, const void* W,
                           int64_t ldw, const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int N,
                           int K, int dtype, int epilogue, void* stream);

/* r04: 1 when v3d_linear_decode_rows with a norm_weight and M rows takes the matrix-core form that normalises the rows itself (more than
 * four rows, K <= 4096, 9..32 K tiles of 128, no residual epilogue; the 1 / rms of a row is formed in v3d_rmsnorm's summation order for
 * that many rows, so the result equals v3d_rmsnorm followed by the unfused call bit for bit), else 0: such a call is then refused for
 * M > 4 and the caller normalises with v3d_rmsnorm first.  Host-only. */
int v3d_linear_decode_rows_fuses_norm(int M, int N, int K, int epilogue);

/* The decode linear over OCP e4m3 weights (BASELINE configs[3]; W8A16): W8 [N,K] bytes (row stride ldw) with one
 * f32 scale per output row as v3d_quantize_fp8_rows writes them; y[m,n] = scale_w[n] * sum_k W8[n,k] x[m,k], then
 * the epilogue of v3d_linear_decode.  K % 16 == 0.  M = 1: VALU form; M = 2..32 with K % 256 == 0, N % 16 == 0: matrix-core
 * form (weights widened to the activation type in registers; a row's result depends neither on the other rows nor on
 * M); other shapes: VALU form, M <= 4.  Not a reference code path (tolerance: tests/test_gpu_fp8.py). */
int v3d_linear_decode_fp8_rows(const void* x, int64_t ldx, int M, const void* W8, int64_t ldw, const float* scale_w,
                               const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int N, int K,
                               int dtype, int epilogue, void* stream);

/* The decode linear over MXFP4 weights (W4A16): Wq [N, K/2] codes (row stride ldw bytes) and We [N, K/32] exponents (row
 * stride lde bytes) as v3d_quantize_mxfp4_rows writes them; y[m,n] = sum_k deq(W)[n,k] x[m,k] with deq(W) widened exactly to
 * the activation type, f32 accumulation, then the epilogue of v3d_linear_decode.  K % 128 == 0.  M = 1: VALU form;
 * M = 2..32 with K % 256 == 0, N % 16 == 0 (SWIGLU: N % 128 == 0), lde % 8 == 0 and We 8-byte aligned: matrix-core form (a
 * row's result depends neither on the other rows nor on M); other shapes: VALU form, M <= 4.  Not a reference code path
 * (tolerance: tests/test_gpu_fp4.py). */
int v3d_linear_decode_mxfp4_rows(const void* x, int64_t ldx, int M, const void* Wq, int64_t ldw, const void* We, int64_t lde,
                                 const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int N, int K,
                                 int dtype, int epilogue, void* stream);

/* Decode-step K14 + cache append in one launch: rotary at position `pos` on the n_q + n_kv heads at the start
 * of the QKV row (in place), rotated k and v copied to cache_row = [k heads | v heads]. */
int v3d_rope_kv_append(void* qkv_row, int n_q_heads, int n_kv_heads, int head_dim, const void* cos_table,
                       const void* sin_table, int n_pos, int pos, void* cache_row, int dtype, void* stream);
/* M = 1..32 scenes in one launch: QKV rows qkv + m*qkv_stride, positions pos[m] and cache rows cache_rows[m] (HOST arrays). */
int v3d_rope_kv_append_rows(void* qkv, int64_t qkv_stride, int M, int n_q_heads, int n_kv_heads, int head_dim,
                            const void* cos_table, const void* sin_table, int n_pos, const int* pos,
                            void* const* cache_rows, int dtype, void* stream);

/* Greedy token choice: index of the maximum of x[0..n) (lowest index on ties, as torch.argmax).
 * workspace: 1 KiB of device scratch. */
int v3d_argmax(const void* x, int n, int dtype, int64_t* out_index, void* workspace, void* stream);
/* M rows x + m*ldx in one launch pair; out_index[M]; workspace >= M KiB. */
int v3d_argmax_rows(const void* x, int64_t ldx, int M, int n, int dtype, int64_t* out_index, void* workspace, void* stream);

/* The stop test of greedy decoding on the device (generate(..., eos_token_id), llava_qwen.py:208-236 -> HF greedy search):
 * done[m] |= tokens[m] in eos_ids[0:n_eos] (device int64 arrays; done: device int32 [M], kept across steps), *n_done = number
 * of rows that have finished.  The host polls n_done asynchronously instead of synchronising on every token. */
int v3d_eos_update(const int64_t* tokens, int M, const int64_t* eos_ids, int n_eos, int32_t* done, int32_t* n_done, void* stream);

/* ------------------------------------------------------------------ beam search (a23, num_beams > 1) - */
/* Added under ABI 7 (no entry changed).  The rule is DESIGN section 2, "Beam search, stated once"; B = num_beams <= 16 (two sets
 * of 16 K/V slices), K = max(2, 1 + n_eos) * B <= 64 candidates per step.
 *
 * v3d_beam_topk: M rows (1: the prefill's row, or B) of 16-bit logits x + b * ldx, V columns; score[b, v] = running[b] +
 * (x[b, v] - lse_b) in f32 (f32 log-sum-exp per row); the K largest as cand_score[K] / cand_flat[K] (flat = b * V + v), descending,
 * equal scores in ascending flat order.  Rows with running[b] <= -1e9 are not read.  done (device int32 word, may be NULL): when
 * set, nothing is written.  workspace: v3d_beam_topk_workspace_bytes(M, V, K), 16-byte aligned.  v3d_beam_topk_chunk: the vocab
 * columns one workgroup selects from (a row is cut at its multiples). */
int64_t v3d_beam_topk_workspace_bytes(int M, int V, int K);
int v3d_beam_topk_chunk(int M, int V);
int v3d_beam_topk(const void* logits, int64_t ldx, int M, int V, int dtype, const float* running, int K, float* cand_score,
                  int32_t* cand_flat, const int32_t* done, void* workspace, int64_t workspace_bytes, void* stream);
/* v3d_beam_step: step `step` (0-based) of the search over the K candidates; one workgroup.  state: v3d_beam_state_bytes(B,
 * max_new_tokens) bytes of 4-byte words laid out as csrc/beam_step.h says (word 0 = done, an int32 WORD that is 0 or 1, not a count;
 * word 1 = the heuristic's flag; word 2 = steps executed; then the running scores, which v3d_beam_topk reads as `running`); the
 * caller initialises it (v3d.ops.beam_state).  div[n] = float32(n ** length_penalty), n <= max_new_tokens (device).  Writes
 * next_tokens int64[B] and parents int32[B] for the next decode step and row `step` of the trace [max_new_tokens, K].  Once done is
 * set the call changes nothing.  v3d_beam_step_host: the same body over host memory. */
int64_t v3d_beam_state_bytes(int B, int max_new_tokens);
int v3d_beam_step(const float* cand_score, const int32_t* cand_flat, int K, int B, int V, int max_new_tokens, int step,
                  const int64_t* eos_ids, int n_eos, const float* div, void* state, int64_t* next_tokens, int32_t* parents,
                  float* trace_score, int32_t* trace_flat, void* stream);
int v3d_beam_step_host(const float* cand_score, const int32_t* cand_flat, int K, int B, int V, int max_new_tokens, int step,
                       const int64_t* eos_ids, int n_eos, const float* div, void* state, int64_t* next_tokens, int32_t* parents,
                       float* trace_score, int32_t* trace_flat);
/* v3d_beam_kv_gather: for every layer l < n_layers (layer_ptrs: DEVICE array of the layers' base pointers, each [n_slices,
 * slice_rows, >= width] 16-bit with the given strides in elements), rows [S, S + n) of slice src_base + parents[b] are copied to
 * slice dst_base + b, b < B, in one launch of 16-byte loads and stores.  The two slice sets must be disjoint.  parents: device
 * int32[B]; done as above. */
int v3d_beam_kv_gather(void* const* layer_ptrs, int n_layers, int64_t slice_stride, int64_t row_stride, int width, int n_slices,
                       int64_t slice_rows, int S, int n, int src_base, int dst_base, int B, const int32_t* parents, const int32_t* done,
                       void* stream);

/* ------------------------------------------------------------------ sampling (do_sample) - */
/* Added under ABI 7 (no entry changed).  The rule is DESIGN section 2, "Sampling, stated once": transformers' temperature, top-k
 * and top-p warpers (min_tokens_to_keep = 1; top_k == 0 and top_p == 1 mean "off"), ties ordered by the lower index, then one
 * Gumbel-max draw per row from Philox4x32-10 at counter (token >> 2, step, stream, 0), key = seed.
 *
 * v3d_sample_rows: M <= 32 rows of 16-bit logits x + m * ldx, V columns, M * V < 2^31.  streams: device int32[M], the rows'
 * stream ids, or NULL for 0 .. M-1.  out_index: device int64[M].  kept (device int32[M], may be NULL): the size of each row's kept
 * set.  A row's token depends on its logits, seed, step and stream only.  workspace: v3d_sample_workspace_bytes(M, V), 16-byte
 * aligned.  v3d_sample_chunk: the vocab columns one workgroup of the draw covers (a row is cut at its multiples).
 * v3d_sample_rows_host: the same rule over f32 logits in host memory (the integer parts are the kernel's bits; the mass of the
 * top-p test is summed in f64 and the keys use the host's logf). */
int64_t v3d_sample_workspace_bytes(int M, int V);
int v3d_sample_chunk(int M, int V);
int v3d_sample_rows(const void* logits, int64_t ldx, int M, int V, int dtype, float temperature, int top_k, float top_p, uint64_t seed,
                    int step, const int32_t* streams, int64_t* out_index, int32_t* kept, void* workspace, int64_t workspace_bytes,
                    void* stream);
int v3d_sample_rows_host(const float* logits, int64_t ldx, int M, int V, float temperature, int top_k, float top_p, uint64_t seed,
                         int step, const int32_t* streams, int64_t* out_index, int32_t* kept);
/* Philox4x32-10 as the sampler uses it (counter[4], key[2] -> out[4]): the known-answer hook of the tests. */
int v3d_philox4x32_10_host(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* ------------------------------------------------------------------ logits processors - */
/* Added under ABI 7 (no entry changed).  The rule is DESIGN section 2, "Logits processors, stated once": transformers'
 * RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor over the tokens generated so
 * far, in that order, applied in place to the 16-bit logits the token choice reads next.
 *
 * v3d_logits_process_rows: M <= 32 rows x + m * ldx of V columns; columns [V, ldx) are never written.  history: device int64, row
 * m's j-th generated token at history[j * ld_step + m] (ld_step >= M), n_prev <= 8192 of them (the step number).  penalty > 0 (1:
 * off): every distinct history id v gets x[v] = round16(x[v] < 0 ? x[v] * penalty : x[v] / penalty), from the unpenalised value,
 * once.  ngram >= 0 (0: off): when n_prev + 1 >= ngram every id that would complete an n-gram already in the history is set to
 * -inf.  min_new >= 0 (0: off): while n_prev < min_new the n_eos ids of eos_ids (device int64) are set to -inf.  Ids outside [0, V)
 * are skipped.  One launch, one workgroup per row, work proportional to n_prev; no launch when nothing applies at this step.
 * v3d_logits_process_rows_host: the same arithmetic (csrc/logits_rule.h) over f32 logits in host memory that hold values of
 * `dtype` (V3D_F16 / V3D_BF16). */
int v3d_logits_process_rows(void* logits, int64_t ldx, int M, int V, int dtype, const int64_t* history, int64_t ld_step, int n_prev,
                            float penalty, int ngram, int min_new, const int64_t* eos_ids, int n_eos, void* stream);
int v3d_logits_process_rows_host(float* logits, int64_t ldx, int M, int V, int dtype, const int64_t* history, int64_t ld_step, int n_prev,
                                 float penalty, int ngram, int min_new, const int64_t* eos_ids, int n_eos);

/* ------------------------------------------------------------------ grounding (K19, K20) - */

/* K19  llava_arch.py:357-372, object_feature_type 'patch14': mask[o, f, py, px] = 1 iff at least `thresh`
 * (= int(14*14*0.5)) pixels of the cell x cell ViT patch lie inside box o = (centre xyz, size xyz);
 * 'patch27' (:367-371): cell = 27 (the pooled 14 x 14 token grid), thresh = int(27*27*0.25); cell * cell <= 768.
 * coords [F,S,S,3] dtype (first S-6 rows/cols used), boxes [n,6] dtype -> mask uint8 [n, F*g*g], g = (S-6)/cell. */
int v3d_object_patch_mask(const void* coords, int dtype, int F, int S, int cell, const void* boxes, int n_obj,
                          int thresh, uint8_t* mask, void* stream);

/* The 'mlp' and 'score' grounding heads (llava_qwen.py:59-86, 283-293; the shipped checkpoints use 'infonce', K20).
 * v3d_row_dots: out[i] = sum_c x[i,c] * q[c] (+ bias[0]); products_rounded != 0: every product is rounded to the dtype first
 * (`(ground_hidden * object_features).sum(dim=-1)`, :285), 0: a Linear(C, 1) row (:81-84).
 * v3d_relu_mul_rows: x[i,c] = relu?(x[i,c]) * (row ? row[c] : 1) in place (nn.ReLU; `obj_feat * query_feat`, :290). */
int v3d_row_dots(const void* x, int64_t ldx, int n_rows, const void* q, int C, const void* bias, int products_rounded,
                 void* out, int dtype, void* stream);
int v3d_relu_mul_rows(void* x, int64_t ldx, int n_rows, int cols, const void* row, int relu, int dtype, void* stream);

/* llava_arch.py:482-501: out[o] = mean of the rows t of feat [T,C] with mask[o,t] != 0 (zeros if none)
 * (+ add[o] if add != NULL: the box-centre PE). */
int v3d_masked_mean(const void* feat, const uint8_t* mask, int n_obj, int T, int C, const void* add, void* out,
                    int dtype, void* stream);

/* K20  predict_box 'infonce', llava_qwen.py:298-300: scores[i] = <normalize(obj[i]), normalize(query)>. */
int v3d_ground_scores(const void* obj, int64_t ldo, int n_rows, const void* query, int C, void* scores, int dtype,
                      void* stream);

/* The same scores for G queries in one launch (one scene's proposals against a batch of grounding queries):
 * scores[g * lds + i] = <normalize(obj[i]), normalize(queries + g * ldq)>, i < n_rows, g < G; grid (n_rows, G).  Every (object, query)
 * pair goes through v3d_ground_scores' own arithmetic, so row g equals v3d_ground_scores(obj, ..., queries + g * ldq, ...) bit for
 * bit.  f16 / bf16, any C > 0, ldo, ldq >= C, lds >= n_rows. */
int v3d_ground_scores_rows(const void* obj, int64_t ldo, int n_rows, const void* queries, int64_t ldq, int G, int C, void* scores,
                           int64_t lds, int dtype, void* stream);

/* ------------------------------------------------------------------ data movement ------- */

/* out[r, 0:cols] = in[r, 0:cols] for strided rows (KV-cache append). */
int v3d_copy_rows(const void* in, int64_t ldi, void* out, int64_t ldo, int64_t rows, int cols, int dtype,
                  void* stream);

/* The same rows to n_copies destinations: out[c*copy_stride + r*ldo + 0:cols] = in[r*ldi + 0:cols], c < n_copies (the cached
 * K/V prefix of a scene handed to the caches of the questions that are answered together; not a reference code path - the
 * reference recomputes the prefix per question, llava/eval/model_scanqa.py:130-185). */
int v3d_copy_rows_bcast(const void* in, int64_t ldi, void* out, int64_t ldo, int64_t rows, int cols, int n_copies,
                        int64_t copy_stride, int dtype, void* stream);

/* a7: SigLipImageProcessor.preprocess, siglip_encoder.py:47-67, for frames that already have the tower's size (the
 * 384 x 384 crops of VideoProcessor.preprocess, video_utils.py:292-308, for which its bicubic resize is the identity):
 * frames [F,H,W,3] u8 (device) -> out [F,3,H,W];  v = f32(f64(u8) * rescale);  out = T((v - mean[c]) / std[c]) in f32. */
int v3d_preprocess_rgb_u8(const uint8_t* frames, int F, int H, int W, const float* mean_host, const float* std_host,
                          double rescale, void* out, int dtype, void* stream);

/* a6 / a7, RGB half: `frame.resize((new_w, crop))` + centre crop of VideoProcessor.preprocess (video_utils.py:285-306), i.e.
 * Pillow's Image.resize for 8-bit RGB with its default BICUBIC filter, reproduced bit for bit (libImaging Resample.c: horizontal
 * pass, 8-bit intermediate, vertical pass; 22-bit fixed-point coefficients; clip8), optionally fused with v3d_preprocess_rgb_u8
 * (SigLipImageProcessor.preprocess, siglip_encoder.py:47-67).
 * frames [F,H,W,3] u8 (device).  The resized image would be OH x OW; only the window (crop_top, crop_left, crop_h, crop_w) of it is
 * computed.  bounds_* [n][2] int32 = (first source index, tap count) and coeffs_* [n][ksize_*] int32 per output column (h, n = OW)
 * / row (v, n = OH): DEVICE arrays holding what Pillow's precompute_coeffs + normalize_coeffs_8bpc produce for (W -> OW) and
 * (H -> OH) (v3d.ops.pil_resample_tables; the double arithmetic stays on the caller's side like dim_t / inv_freq do).
 * out_dtype V3D_U8_HWC: out [F,crop_h,crop_w,3] u8 (mean / std may be null);  V3D_F32 / F16 / BF16: out [F,3,crop_h,crop_w] =
 * T((f32(f64(u8) * rescale) - mean[c]) / std[c]).  At most 32 taps per pass (reductions up to ~7x). */
int v3d_resize_bicubic_u8(const uint8_t* frames, int F, int H, int W, int OH, int OW, const int32_t* bounds_h,
                          const int32_t* coeffs_h, int ksize_h, const int32_t* bounds_v, const int32_t* coeffs_v, int ksize_v,
                          int crop_top, int crop_left, int crop_h, int crop_w, const float* mean_host, const float* std_host,
                          double rescale, void* out, int out_dtype, void* stream);

/* K10 input: SigLipVisionEmbeddings' Conv2d(kernel = stride = patch), siglip_encoder.py:156-172, as a
 * GEMM: gathers images [B,3,S,S] into rows [B*(S/patch)^2, kpad], columns (c, ky, kx) zero padded. */
int v3d_patchify(const void* images, void* out, int B, int S, int patch, int kpad, int dtype, void* stream);

/* ------------------------------------------------------------------ training step (configs[4], first kernels) --- */

/* The loss of Qwen2ForCausalLM.forward, llava/model/language_model/qwen2/modeling_qwen2.py:1195-1205: logits [positions, vocab]
 * (dtype: f32 as the reference's `.float()`, or 16-bit; row stride ld), labels [positions] int64 (device); position t predicts
 * label t + 1 (the shift), rows whose label is ignore_index (-100) do not count.  Outputs (device, f32): loss_rows[positions-1]
 * (0 for ignored rows), lse_rows[positions-1] (log-sum-exp per row, reused by the gradient), mean_count[2] = {mean loss over the
 * valid rows (CrossEntropyLoss reduction 'mean'; NaN if none), number of valid rows}. */
int v3d_cross_entropy(const void* logits, int64_t ld, int dtype, int64_t positions, int vocab, const int64_t* labels,
                      int64_t ignore_index, float* loss_rows, float* lse_rows, float* mean_count, void* stream);
/* d loss / d logits: dlogits[t, :] = (softmax(logits[t, :]) - onehot(labels[t + 1])) * upstream / #valid, zero rows for ignored
 * labels and for the last position; written in grad_dtype (the logits' dtype or f32), row stride ldg. */
int v3d_cross_entropy_grad(const void* logits, int64_t ld, int dtype, int64_t positions, int vocab, const int64_t* labels,
                           int64_t ignore_index, const float* lse_rows, const float* mean_count, float upstream, void* dlogits,
                           int64_t ldg, int grad_dtype, void* stream);

/* Backward of v3d_visual_tokens (flags POOL [| PE] [| NEWLINE]) with respect to its parameter-free inputs: the PE add passes the
 * gradient through (llava_arch.py:515: coords are detached), get_2dPool's bilinear 27 -> 14 (llava_arch.py:191-210) scatters
 * it back onto the projector features with the forward's own tap weights (gather form, f32 accumulation in a fixed order), and
 * image_newline (llava_arch.py:307-328) collects the sum of its V * n rows.
 * dout rows as the forward wrote them (V*n*(n+1) with NEWLINE else V*n*n; row stride dout_stride), dfeat [V, side*side, C] dtype,
 * dnewline [C] f32 (NEWLINE only). */
int v3d_visual_tokens_grad(const void* dout, int64_t dout_stride, void* dfeat, float* dnewline, int dtype, int V, int side, int n,
                           int C, int flags, void* stream);

/* Backward of the decoder's dense blocks (r02).  With y = x . W^T (nn.Linear), dx = dy . W and dW = dy^T . x are v3d_gemm calls on
 * transposed operands (v3d/train.py: linear_backward), so the data movement the backward adds is this transpose:
 * out[c, r] = x[r, c] for x [rows, cols] (16-bit; cols % 8 == 0); columns [rows, out_cols) of out are zero-filled (out_cols % 8 == 0:
 * the k padding of the dW product, whose k runs over token rows). */
int v3d_transpose(const void* x, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t out_cols, int dtype,
                  void* stream);
/* Column sums in f32 with a fixed summation order (32-row partials in `workspace`, then the partials in order): the bias gradient
 * of nn.Linear (sum over token rows of dy).  workspace: v3d_colsum_workspace_bytes(rows, cols) bytes; out [cols] in out_dtype. */
int64_t v3d_colsum_workspace_bytes(int64_t rows, int cols);
int v3d_colsum(const void* x, int64_t ldx, int64_t rows, int cols, int dtype, float* workspace, void* out, int out_dtype, void* stream);
/* Backward of v3d_rmsnorm (Qwen2RMSNorm, modeling_qwen2.py:76-90): with r = rsqrt(mean(x^2) + eps), n = T(x r), g = dy * weight:
 * dx = r (g - n mean(g n)), dweight = sum over rows of dy n (f32, fixed order; workspace as v3d_colsum's).  `add` (may be null):
 * a 16-bit gradient of the same shape added to dx - the residual branch that by-passes the norm (modeling_qwen2.py:771-789). */
int v3d_rmsnorm_grad(const void* x, int64_t ldx, const void* weight, const void* dy, int64_t ldy, const void* add, int64_t lda,
                     void* dx, int64_t ldd, float* workspace, void* dweight, int dw_dtype, int64_t rows, int cols, float eps, int dtype,
                     void* stream);
/* Qwen2MLP's act_fn(gate_proj(x)) * up_proj(x) (modeling_qwen2.py:177-189) on planar rows gu = [gate (inter) | up (inter)]
 * (the training forward keeps gate / up for the backward; the inference path forms the product in v3d_gemm's SWIGLU epilogue):
 * out = T(T(silu(g)) * u); the gradient dgu = [dh u silu'(g) | dh silu(g)]. */
int v3d_swiglu(const void* gu, int64_t ld, void* out, int64_t ldo, int64_t rows, int inter, int dtype, void* stream);
int v3d_swiglu_grad(const void* gu, int64_t ld, const void* dh, int64_t ldh, void* dgu, int64_t ldg, int64_t rows, int inter,
                    int dtype, void* stream);

/* Attention backward, first form: one head's probabilities are materialised (16-bit [queries, keys], the rounding points of the
 * reference's eager attention, modeling_qwen2.py:248-327) and the five products run on v3d_gemm (v3d/train.py: attention_backward);
 * these are the two row passes between them.  cols = the padded key count (% 8 == 0, <= 8192).
 * v3d_causal_softmax_rows: p[i, j] = softmax over the keys j <= i + offset, j < n_keys of T(s[i, j] * scale); 0 for the other j < cols.
 * v3d_softmax_grad_rows:   ds[i, j] = T(p (dp - sum_j p dp)) * scale (rounded to T). */
int v3d_causal_softmax_rows(const void* s, int64_t lds, void* p, int64_t ldp, int64_t rows, int n_keys, int cols, int offset,
                            float scale, int dtype, void* stream);
int v3d_softmax_grad_rows(const void* p, int64_t ldp, const void* dp, int64_t ldd, void* ds, int64_t lds, int64_t rows, int cols,
                          float scale, int dtype, void* stream);

/* Attention backward as tiled kernels (the [S, S] matrices never reach HBM): v3d_attention_train is v3d_attention at head dim 128
 * (outputs bit-identical) that also writes lse [B, Hq, Sq] f32, the row log-sum-exp in the kernel's scaled log2 units;
 * v3d_attention_backward (Sq = Sk = S, heads 128 columns apart inside a token row, B sequences with element strides bs*; causal =
 * the decoder, modeling_qwen2.py:248-482, non-causal = the SigLIP encoder with its 72-wide heads zero-padded to 128,
 * siglip_encoder.py:197-250) recomputes the probabilities from q, k and lse and writes dq [S, Hq 128], dk, dv [S, Hkv 128] per sequence
 * (the sum over a kv group's query heads is taken in f32, in a fixed order: no atomics).  q / k are what the forward multiplied (the
 * ROTATED projections in the decoder), o the forward's output, dout its gradient.  workspace:
 * v3d_attention_backward_workspace_bytes(B, S, Hq) bytes. */
int v3d_attention_train(const void* q, const void* k, const void* v, void* o, float* lse, int dtype, int B, int Sq, int Sk, int Hq,
                        int Hkv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t bsq, int64_t bsk, int64_t bso, int hsq,
                        int hsk, int hso, int causal, int q_pos0, float scale, void* stream);
int64_t v3d_attention_backward_workspace_bytes(int B, int S, int Hq);
int v3d_attention_backward(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                           void* dk, void* dv, int dtype, int B, int S, int Hq, int Hkv, int64_t ldq, int64_t ldk, int64_t ldv,
                           int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, int64_t bsq, int64_t bsk, int64_t bsv,
                           int64_t bso, int64_t bsdo, int64_t bsdq, int64_t bsdk, int64_t bsdv, int causal, float scale,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* One AdamW update of a flat parameter tensor (torch.optim.AdamW's single-tensor form = the reference's HF Trainer optimizer; ZeRO
 * runs the same update on its f32 master partition): p32 / m / v [n] f32 in place, grad [n] in grad_dtype (f32 / f16 / bf16) times
 * grad_scale, p16 (may be null) the 16-bit copy the next forward reads.  step counts from 1 (bias correction). */
int v3d_adamw_step(float* p32, float* m, float* v, const void* grad, int grad_dtype, void* p16, int p16_dtype, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* Gradient of the embedding lookup for the text rows of a sample (llava_arch.py:650-700 embeds them with embed_tokens):
 * dE[ids[i], :] = sum over the j with ids[j] == ids[i], in order, of dh[rows[j], :] (f32 sums, one rounding); rows / ids: device
 * int64 [n].  Rows of dE that no id names are not touched (the caller zero-fills).
 * dh has n_rows rows, dE vocab rows: ids outside [0, vocab) (a raw prompt's IMAGE_TOKEN_INDEX = -200) and rows outside
 * [0, n_rows) are skipped - nothing is read or written for them. */
int v3d_embed_grad(const void* dh, int64_t ld, int64_t n_rows, const int64_t* rows, const int64_t* ids, int n, int H, void* dE, int64_t lde,
                   int64_t vocab, int dtype, void* stream);

/* GELU as a pass of its own for the training forward (which keeps the pre-activation z) and its gradient dz = dy * gelu'(z):
 * tanh_form 0 = nn.GELU() of the mm_projector (multimodal_projector/builder.py:41-48), 1 = gelu_pytorch_tanh of the SigLIP MLP
 * (siglip_encoder.py:253-262), 2 = nn.ReLU() of the grounding heads (llava_qwen.py:99-110; z may be the ReLU's output).  f32 inside,
 * one rounding. */
int v3d_gelu(const void* z, int64_t ldz, void* out, int64_t ldo, int64_t rows, int cols, int tanh_form, int dtype, void* stream);
int v3d_gelu_grad(const void* z, int64_t ldz, const void* dy, int64_t ldy, void* dz, int64_t ldo, int64_t rows, int cols, int tanh_form,
                  int dtype, void* stream);

/* Backward of v3d_layernorm (nn.LayerNorm of the SigLIP encoder layers, siglip_encoder.py:272-274,292,300): with xh = (x - mean) rstd
 * and g = dy * weight: dx = rstd (g - mean(g) - xh mean(g xh)) (+ add, the residual branch's gradient), dweight = sum_rows dy xh,
 * dbias = sum_rows dy (f32, fixed order).  workspace: 2 * v3d_colsum_workspace_bytes(rows, cols) bytes.  cols <= 3584. */
int v3d_layernorm_grad(const void* x, int64_t ldx, const void* weight, const void* dy, int64_t ldy, const void* add, int64_t lda, void* dx,
                       int64_t ldd, float* workspace, void* dweight, void* dbias, int dw_dtype, int64_t rows, int cols, float eps,
                       int dtype, void* stream);

/* y[i] = T(y[i] + alpha * x[i]) for flat 16-bit tensors: gradient accumulation over micro-batches (train_multi.sh:31-32, 60:
 * gradient_accumulation_steps = 2), in the arithmetic torch uses when it adds a new gradient to .grad (f32 add, one rounding). */
int v3d_axpy(void* y, const void* x, float alpha, int64_t n, int dtype, void* stream);

/* Sum of squares of a flat tensor x [n] (f32 / f16 / bf16; 16-byte aligned) in f32 -> out[0] (device; accumulate != 0: added to it),
 * deterministic (fixed partials folded in a fixed order).  The global gradient norm of gradient clipping - the HF Trainer's
 * max_grad_norm = 1.0 behind scripts/zero2.json:36 "gradient_clipping": "auto" and torch.nn.utils.clip_grad_norm_ - is the square root
 * of the sum of these over the gradient tensors.  workspace: v3d_sumsq_workspace_bytes() bytes of device scratch. */
int64_t v3d_sumsq_workspace_bytes(void);
int v3d_sumsq(const void* x, int64_t n, int dtype, float* out, int accumulate, float* workspace, void* stream);

/* The grounding loss (ScanRefer / Multi3DRefer samples of the joint training), predict_box 'infonce', llava_qwen.py:296-310: with
 * s_i = <normalize(obj[i]), normalize(query)> (v3d_ground_scores) over the n head outputs obj [n, C] (the zero-target row included),
 * loss = -log(sum_{positive i} e^{s_i / temperature} / sum_i e^{s_i / temperature}); positive: device uint8 [n].  Writes loss (f32
 * scalar), scores (f32 [n], may be null) and the gradients dobj [n, C], dquery [C].  n <= 1024. */
int v3d_ground_infonce(const void* obj, int64_t ldo, int n, const void* query, int C, const uint8_t* positive, float temperature,
                       float* loss, float* scores, void* dobj, int64_t ldd, void* dquery, int dtype, void* stream);
/* Backward of v3d_masked_mean (llava_arch.py:482-501): dfeat[t, :] = (accumulate ? dfeat[t, :] : 0) + sum over the objects o with
 * mask[o, t] != 0, in order, of dobj[o, :] / count[o]; dfeat [T, C] contiguous, inv_count: f32 [n_obj] scratch. */
int v3d_masked_mean_grad(const uint8_t* mask, int n_obj, int T, int C, const void* dobj, void* dfeat, int accumulate, float* inv_count,
                         int dtype, void* stream);

/* The grounding loss of the 'mlp' and 'score' heads (llava_qwen.py:283-293, 313-322), the heads' score tail and its backward in one
 * launch: s_i = sum_c x[i,c] w[c] (+ bias[0]; products_rounded != 0: every product rounded to the dtype first, as v3d_row_dots),
 * with t_i = positive[i] != 0 and weight_i = t_i ? pos_weight : 1, loss = mean_i weight_i (max(s_i,0) - s_i t_i + log1p(e^-|s_i|))
 * (BCEWithLogitsLoss(reduction='none') * weight, .mean(); f32 inside).  Writes loss (f32 scalar), scores (f32 [n], may be null),
 * dx [n, C] = ds (x) w, dw [C] = sum_i ds_i x[i,:], dbias [1] = sum_i ds_i (may be null), ds_i = weight_i (sigmoid(s_i) - t_i) / n.
 * pos_weight is the host's (n - P) / P of the P listed labels (ground_bce_targets).  One workgroup, sums in a fixed order (two calls
 * give identical bits).  1 <= n <= 1024, C a multiple of 8 up to 3584, rows 16-byte aligned, dx distinct from x. */
int v3d_ground_rowdot_bce(const void* x, int64_t ldx, int n, const void* w, int C, const void* bias, int products_rounded,
                          const uint8_t* positive, float pos_weight, float* loss, float* scores, void* dx, int64_t lddx, void* dw,
                          void* dbias, int dtype, void* stream);
/* Backward of m = o * q_row (v3d_relu_mul_rows with a row, relu 0; `obj_feat * query_feat`, llava_qwen.py:290): dout[i,:] = dm[i,:] * q
 * (one rounding), dq[c] = sum_i dm[i,c] o[i,c] in f32, rows in order.  C a multiple of 8, rows 16-byte aligned. */
int v3d_mul_rows_grad(const void* dm, int64_t lddm, const void* o, int64_t ldo, const void* q, int n, int C, void* dout, int64_t lddo,
                      void* dq, int dtype, void* stream);

/* ------------------------------------------------------------------ LoRA rank products -- */

/* The products of a LoRA-adapted Linear in which one dimension is the rank (peft's LoraLayer; llava/train/train_3d.py:168-173,
 * 259-274: lora_r 64, lora_alpha 16 on the decoder's seven linears): for W [N, K], A [r, K], B [N, r], s = lora_alpha / r,
 *   forward   u = x A^T (rounded), y = x W^T (+ bias) + s u B^T
 *   backward  du = s dy B (rounded), dB = s dy^T u, dA = du^T x, dx = dy W + du A, no dW.
 * Both entries take 16-bit operands (V3D_F16 / V3D_BF16), R % 16 == 0 with 16 <= R <= 384 (R = the rank, or the stacked rank of fused
 * q|k|v and gate|up rows), K % 64 == 0, any M >= 1, row strides that are multiples of 8, 16-byte aligned pointers and operands that span
 * fewer than 2^31 elements; every argument check runs before any device call.  Nothing outside [M, R] resp. [R, K] of the outputs is
 * written and nothing outside [M, K], [R, K], [M, R] of the operands is read.
 *
 * v3d_lora_down: out[M, R] = T(scale * X[M, K] . P[R, K]^T), f32 accumulation with k ascending in one run per output, one f32 product
 * with scale, one rounding.  u = x A^T (P = A, scale 1) and du = s dy B (P = B^T [r, N], a transposed copy by v3d_transpose). */
int v3d_lora_down(const void* X, int64_t ldx, const void* P, int64_t ldp, float scale, void* out, int64_t ldo, int64_t M, int R, int K,
                  int dtype, void* stream);
/* v3d_lora_wgrad: G[R, K] = scale * U[M, R]^T . X[M, K] in g_dtype (f32, or 16 bit with one rounding); the sum runs over the M rows and
 * both operands are read as stored.  dA = du^T x (U = du, X = x) and dB^T = s u^T dy (U = u, X = dy, scale s).  The rows are cut into
 * chunks of v3d_lora_wgrad_chunk(M, R, K) rows (a multiple of 32); each workgroup sums one chunk in row order for 64 columns and stores
 * an f32 partial into workspace, and a second launch adds the partials in chunk order, multiplies by scale and rounds: no atomics, two
 * calls give identical bits.  workspace: v3d_lora_wgrad_workspace_bytes(M, R, K) bytes from the caller (both are pure functions of the
 * shape, host only, 0 for a shape the kernel does not take; neither decreases when M grows). */
int64_t v3d_lora_wgrad_chunk(int64_t M, int R, int K);
int64_t v3d_lora_wgrad_workspace_bytes(int64_t M, int R, int K);
int v3d_lora_wgrad(const void* U, int64_t ldu, const void* X, int64_t ldx, float scale, void* G, int64_t ldg, int g_dtype, int64_t M, int R,
                   int K, int dtype, float* workspace, void* stream);

/* ------------------------------------------------------------------ host helpers -------- */

/* The launch plan v3d_gemm takes for an M x N x K product on a chip with `slots` compute units (pure host code, no device needed;
 * defaults of the V3D_GEMM_* switches): *kernel 0 = skinny (M <= 8), 1 = 128 x 128 tile, 2 = 256 x 256 ping-pong, 3 = 192 x 256
 * ping-pong; *tiles of that kernel; with the split-K tail (kernel 2 only) *dp = whole-tile rounds and *split = K-chunks per left-over
 * tile (2..4), else *dp = -1, *split = 1.  Invariants a test can hold it to: (tiles - dp * (slots & ~7)) * split <= slots & ~7 (every
 * chunk has a workgroup), K / 64 even and K / 128 >= 2 * split (a chunk is at least two 2-K-step granules). */
int v3d_gemm_plan_host(int M, int N, int K, int slots, int* kernel, int* tiles, int* dp, int* split);

/* a1  llava/video_utils.py:187  np.linspace(0, total-1, n, dtype=int).  out_host[n]. */
int v3d_uniform_frame_indices_host(int total_frames, int n, int32_t* out_host);

/* a3  scripts/3d/preprocessing/max_coverage_sampling.py:44-94 greedy max-coverage with the tie
 * rule "lowest frame position" (the reference draws random.choice, unseeded, :84).
 * keys_host [n_frames, pts_per_frame, 3] int32 voxel keys (round(xyz/voxel)), scene_host [m,3]
 * int32 scene voxel set.  Writes up to max_frames picks: sel_host (frame positions), gain_host
 * (voxel_nums), and the two totals.  Returns the number of picks or a negative error. */
int v3d_greedy_cover_host(const int32_t* keys_host, int n_frames, int64_t pts_per_frame,
                          const int32_t* scene_host, int64_t m, int max_frames, int32_t* sel_host,
                          int64_t* gain_host, int64_t* num_all_host, int64_t* num_sel_host);

/* ------------------------------------------------------------------ a3 on the device ---- */

/* scripts/3d/preprocessing/max_coverage_sampling.py:44-45: keys = round(xyz / voxel_size) as int32 (f32 division,
 * round half to even).  xyz / keys: n_values scalars (3 per point), device. */
int v3d_voxel_keys_f32(const float* xyz, int64_t n_values, float voxel_size, int32_t* keys, void* stream);

/* The greedy max-coverage loop of max_coverage_sampling.py:46-94 on the device, same contract and tie rule as
 * v3d_greedy_cover_host.  keys [n_frames, pts_per_frame, 3] and scene [m,3] int32 in HBM; outputs in HBM:
 * sel[max_frames] (frame positions), gain[max_frames] (voxel_nums), totals[2] = {num_all_voxels, num_select_voxels},
 * n_sel[1] = number of picks.  Stream-ordered, no host synchronisation.  Coordinates must lie in [-2^20, 2^20): a
 * scene key outside sets the int at workspace byte offset (workspace_bytes_needed - 256) to 1 (the wrapper raises);
 * frame keys outside can never match a scene voxel and are ignored. */
int64_t v3d_greedy_cover_workspace_bytes(int n_frames, int64_t m);
int v3d_greedy_cover(const int32_t* keys, int n_frames, int64_t pts_per_frame, const int32_t* scene, int64_t m,
                     int max_frames, int32_t* sel, int64_t* gain, int64_t* totals, int32_t* n_sel, void* workspace,
                     int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* V3D_H_ */
