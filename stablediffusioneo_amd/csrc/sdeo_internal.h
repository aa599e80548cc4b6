/* Private entry points of libsdeo.so: tuning and measurement hooks used by tools/ and a few op tests.  NOT part of the
 * drop-in boundary (include/sdeo.h): nothing a reference-side binding needs is declared here. */
#ifndef SDEO_INTERNAL_H
#define SDEO_INTERNAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* force tile config / split-K of the following conv/GEMM launches (-1, 0 = plan table / heuristic) */
void sdeo_debug_force_gemm_plan(int tile, int splitk);
void sdeo_debug_force_gemm_order(int order); /* -1 heuristic, 0 M-fastest, 1 N-fastest tile order within an XCD */
/* name of the kernel instantiation sdeo_conv2d_nhwc_f16 would launch for this problem (plan table / forced plan / heuristic) */
const char* sdeo_debug_conv2d_kernel_name(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x);
/* name of the kernel instantiation sdeo_attention_f16 / sdeo_attention_causal_f16 would launch for this shape, template arguments as
 * the device symbol carries them ("attention_kernel<3,2,true,4>": D16, KS, MPAD, QB; "attention_wide_kernel<128>"), formatted from
 * the launcher's own selection.  NULL, with sdeo_last_error set, for a shape the launch rejects (head dim).  Host only, no device call;
 * the string is valid until the calling thread's next query. */
const char* sdeo_debug_attention_kernel_name(int B, int H, int Tq, int Tk, int d, int causal);
/* the same for sdeo_attention2_f16 ("attention2_kernel<3,true>": D16, MPAD; the two-segment forms of attention_kernel<D16,1,MPAD,4>).
 * NULL, with sdeo_last_error set, for a shape the launch rejects (head dim, Tk2 outside 1..64). */
const char* sdeo_debug_attention2_kernel_name(int B, int H, int Tq, int Tk, int Tk2, int d);
/* the checks sdeo_attention2_f16 makes before its launch, alone (same arguments without the stream): 0 when the call would launch, else
 * its refusal with sdeo_last_error set.  Host only: no device call is made and no operand is read, so a test may pass any address. */
int sdeo_debug_attention2_check(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk, int tk_stride,
                                int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2, int tk2_stride,
                                int v2_batch_stride, float weight2, int b, int heads, int tq, int d, float scale);
/* plan queries (tests; host only, no device call): the problem of an sdeo_conv2d_nhwc_f16 / sdeo_gemm_f16 call of this shape with
 * `act` and, for fp8 != 0, fp8 weights -> the tuned-table key it looks up (key10) and the (tile, split-K) it would launch */
int sdeo_debug_conv2d_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int act, int fp8, int* key10,
                           int* tile, int* splitk);
int sdeo_debug_gemm_plan(int m, int n, int k, int act, int fp8, int* key10, int* tile, int* splitk);
/* multi-problem launch (csrc/conv_gemm.hip, conv_gemm_dma_kernel MULTI): `count` GEMMs y_i = scale_i * (x_i w_i^T + bias_i) + res_i
 * (fp16, row strides in elements, bias_i / res_i may be NULL) as ONE unsplit launch.  Arrays of `count` entries; the pointer arrays
 * hold device pointers.  tile_i / splitk_i: the plan forced on problem i (as sdeo_debug_force_gemm_plan forces one launch; splitk 0 or
 * 1 = unsplit); the launch runs on tile_0.  Refused on the host, before any device call: count > 16, a split-K plan, tiles that differ
 * ("mixed tiles"), a tile without a multi-problem instantiation. */
int sdeo_debug_gemm_multi_f16(int count, const int* tile, const int* splitk, const int* m, const int* n, const int* k, void* const* y,
                              const int* ldy, const void* const* x, const int* ldx, const void* const* w, const int* ldw,
                              const void* const* bias, const void* const* res, const int* ldres, const float* scale, void* stream);
/* (tile, split-K) of the last conv / GEMM launch (host-side record; -1 / 0 before the first) */
void sdeo_debug_last_gemm_plan(int* tile, int* splitk);
/* epilogue kind of that launch (csrc/conv_inl.h: EpiKind): 0 the staged family (the generic kernel and every specialisation of it),
 * 1 stored from the accumulators; -1 before the first */
int sdeo_debug_last_gemm_epilogue(void);
/* the staged mode of that launch: 0 the generic kernel (and every direct launch), else the EpiKind of the specialised kernel:
 * 2 split-K slabs, 3 GEGLU pair, 4 GroupNorm partials, 5 GroupNorm partials with a per-image bias2 */
int sdeo_debug_last_gemm_epilogue_mode(void);
/* -1 automatic, 0 every non-direct launch runs the generic staged kernel (process-wide, as SDEO_EPI_KINDS=0): A/B inside one process */
void sdeo_debug_force_gemm_epilogue_mode(int mode);
/* 1 when row `tile` of the tile table has the specialised kernel of staged mode `mode` (0: the generic kernel).  Host only. */
int sdeo_debug_tile_has_epilogue_mode(int tile, int mode);
/* the conv / GEMM launches dispatched since the last clear, as rows of six ints (tile, split-K, operand form, EpiKind run, mode flags,
 * count) written to rows6 (room for `cap` rows); returns the number of rows.  form: 0 plain, 1 folded Upsample, 2 fp8 weights,
 * 3 block-scaled fp8, 4 multi-problem.  flags: act | 8 bias2 | 16 GroupNorm partials | 32 row statistics | 64 LayerNorm fold |
 * 128 residual | 256 coalesced epilogue.  Host-side counters (launches under graph replay are not seen).  tools/epilogue_census.py */
int sdeo_debug_gemm_epilogue_census(int* rows6, int cap, int clear);
/* row `tile` of the conv / GEMM tile table (csrc/conv_gemm.hip: kTiles); returns non-zero past the end.  kind: 0 LDS-DMA implicit GEMM,
 * 1 register-staged fallback, 2 halo-reuse 3x3.  caps: 1 four-wave, 2 grouped barrier, 4 has an fp8-weight instantiation,
 * 8 has a block-scaled-fp8 instantiation, 16 halo.  Host only. */
int sdeo_debug_tile_info(int tile, int* kind, int* bm, int* bn, int* stages, int* caps, const char** name);
/* measurement builds only (python -m stablediffusioneo_amd.build --debug, SDEO_DBG_GEMM bit 6): per-workgroup phase stamps of
 * the last GEMM (which = 0) / halo conv (1) launch, 8 x uint64 per workgroup in 10 ns units */
int sdeo_debug_read_stamps(int which, unsigned long long* out, int n);
/* y = silu(x) on n fp16 elements: launch-floor probe for tools/launch_floor.py */
int sdeo_debug_silu(void* y, const void* x, int64_t n, void* stream);

/* op-level hooks of csrc/norm.hip (tests).
 * groupnorm_path: what sdeo_groupnorm_nhwc_f16 launches for this shape, from the launcher's own selection: 0 = two launches
 *   (statistics, apply), 256 / 1024 = the single-launch kernel with that many threads; -1, with sdeo_last_error set, for a shape the
 *   launch rejects.  Host only, no device call.
 * groupnorm_ld / layernorm_ld: sdeo_groupnorm_nhwc_f16 / sdeo_layernorm_f16 on channel blocks of wider buffers: row strides ldx / ldy
 *   in elements (multiples of 8, >= c), as the networks' views pass them
 * softmax_rows: p[r][0:cols] (fp16, row stride ldp) = softmax(s[r][0:cols] * scale) of fp32 scores (row stride lds): the VAE
 *   AttnBlock's materialised-score path */
int sdeo_debug_groupnorm_path(int n, int hw, int c, int groups);
int sdeo_debug_groupnorm_ld_f16(void* y, int ldy, const void* x, int ldx, const float* gamma, const float* beta, int n, int hw, int c,
                                int groups, float eps, int with_silu, void* workspace, void* stream);
int sdeo_debug_layernorm_ld_f16(void* y, int ldy, const void* x, int ldx, const float* gamma, const float* beta, int rows, int c,
                                float eps, void* stream);
int sdeo_debug_softmax_rows(void* p, int ldp, const float* s, int lds, int rows, int cols, float scale, void* stream);

/* op-level hooks for the LayerNorm fold (tests): the networks use these paths internally (csrc/net_build.hip build_attn).
 * fold: w_out = fp16(w * gamma) [rows][c], s_out[rows] = row sums of w_out, b_out[rows] = bias + w beta (bias may be NULL)
 * gemm_stats: sdeo_gemm_f16 (fp16 out) that also writes per-row (sum, sumsq) partials of y: stats fp32 [m][stats_ld][2];
 *   *strips_out = valid partials per row (0: the plan is split-K and cannot emit them; nothing was launched)
 * gemm_ln: y = act(LN(x) w^T + b) given the FOLDED w / s / b and the statistics of x; eps as nn.LayerNorm
 * row_stats: one (sum, sumsq) partial per row of x */
int sdeo_debug_fold_layernorm(void* w_out, float* s_out, float* b_out, const void* w, const float* gamma, const float* beta,
                              const float* bias, int rows, int c, void* stream);
/* [ (Wp W2) | Wp ] (fp16 [c][k2 + c]) and Wp b2 + bp (fp32 [c]): ff.net.2 and proj_out of a SpatialTransformer as one Linear */
int sdeo_debug_compose_proj(void* w_out, float* b_out, const void* wp, const float* bp, const void* w2, const float* b2, int c, int k2,
                            void* stream);
int sdeo_debug_gemm_stats_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                              int ldres, int m, int n, int k, float* stats, int stats_ld, int* strips_out, void* stream);
int sdeo_debug_gemm_ln_f16(void* y, int ldy, const void* x, int ldx, const void* w_folded, int ldw, const float* ln_s,
                           const float* bias_folded, const float* stats, int stats_ld, int strips, int ln_c, int m, int n, int k, int act, float eps, void* workspace, size_t workspace_bytes, void* stream);
int sdeo_debug_row_stats_f16(float* stats, int stats_ld, const void* x, int ldx, int rows, int c, void* stream);
/* [conv whose epilogue emits the GroupNorm partials of its output] -> [normalise-only GroupNorm]: the pair csrc/net_build.hip builds for
 * every conv that feeds a GroupNorm.  *slots = partial entries per image (0: this shape's plan cannot emit them, nothing ran);
 * partials >= n * slots * groups * 2 floats (+ n * groups * 2 when slots > 128) */
int sdeo_debug_conv2d_gn_f16(void* ynorm, void* y, const void* x, const void* w_krsc, const float* bias, const void* res, int n, int h,
                             int w, int cin, int cout, int ksize, int stride, int upsample2x, const float* gamma, const float* beta,
                             int groups, float eps, int with_silu, float* partials, size_t partial_floats, int* slots, void* stream);
/* the same with a per-image bias2 ([n][cout] fp32, NULL = none) added before the store: the ResBlock in_layers conv + time embedding */
int sdeo_debug_conv2d_gn_b2_f16(void* ynorm, void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                                int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, const float* gamma,
                                const float* beta, int groups, float eps, int with_silu, float* partials, size_t partial_floats, int* slots,
                                void* stream);

/* op-level hooks of the shared prefix of the CFG pair (tests; csrc/net_build.hip build_attn): operands that a full-batch launch reads from a
 * half-batch tensor.
 * gemm_res_rows: sdeo_gemm_f16 (fp16 out) whose residual holds res_rows rows (m / 2 <= res_rows <= m): output row r adds residual
 *   row r - res_rows when r >= res_rows.  stats != NULL: also the per-row partials as sdeo_debug_gemm_stats_f16, except that with a
 *   split-K plan (*strips_out = 0) the GEMM still runs and the caller takes the statistics from sdeo_debug_row_stats_f16
 * attention_qb: sdeo_attention_f16 whose q holds q_batches batches (b / 2 <= q_batches <= b): batch i reads the queries of batch
 *   i - q_batches when i >= q_batches; k, v and o hold b batches */
int sdeo_debug_gemm_res_rows_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                                 int ldres, int res_rows, int m, int n, int k, float* stats, int stats_ld, int* strips_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* conv2d_ex: sdeo_conv2d_nhwc_f16 (stride 1, fp16 out) with a residual of res_rows rows (0: one per output row), per-row (sum, sumsq)
 *   partials out (stats != NULL; *strips_out = partials per row) and a LayerNorm-folded input (ln_stats != NULL), which the launch
 *   refuses on the host for filters larger than 1x1 */
int sdeo_debug_conv2d_ex_f16(void* y, const void* x, const void* w_krsc, const float* bias, const void* res, int res_rows, int n, int h,
                             int w, int cin, int cout, int ksize, float* stats, int stats_ld, int* strips_out, const float* ln_stats,
                             const float* ln_s, int ln_ld, int ln_strips, void* workspace, size_t workspace_bytes, void* stream);
/* conv2d_view: sdeo_conv2d_pad_nhwc_f16 on views of wider buffers, as csrc/net_build.hip runs the decoder convs into a concat buffer:
 *   x is a channel block of [n * h * w][ldx], y and res are column blocks of [n * ho * wo][ldy] / [ldres] (tests).  The leading dimensions
 *   and the alignment of the three pointers are checked by the launcher alone (csrc/conv_gemm.hip: prepare) */
int sdeo_debug_conv2d_view_f16(void* y, int ldy, const void* x, int ldx, const void* w_krsc, const float* bias, const float* bias2,
                               const void* res, int ldres, int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x,
                               int pad_before, int pad_after, int act, float scale, void* workspace, size_t workspace_bytes, void* stream);
int sdeo_debug_attention_qb_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                                int q_batches, int heads, int tq, int tk, int tk_stride, int v_batch_stride, int d, float scale, void* stream);
/* attention2_qb: sdeo_attention2_f16 with the same query sharing (k, v, k2, v2 and o hold b batches) */
int sdeo_debug_attention2_qb_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk,
                                 int tk_stride, int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2,
                                 int tk2_stride, int v2_batch_stride, float weight2, int b, int q_batches, int heads, int tq, int d,
                                 float scale, void* stream);

/* fp8 weight pack at op level (tests): quantise [rows][cols] fp16 in place to its dequantised values, codes -> q, scales -> scale;
 * sdeo_debug_next_weights_fp8 makes the NEXT conv / GEMM call of this thread (sdeo_gemm_f16, sdeo_conv2d_nhwc_f16, sdeo_conv2d_pad_nhwc_f16,
 * sdeo_debug_gemm_stats_f16, _gemm_res_rows_f16, _gemm_ln_f16, _conv2d_ex_f16, _conv2d_view_f16, _conv2d_gn_f16, _conv2d_gn_b2_f16) stream these codes
 * (K-contiguous bytes, same [N][K] / KRSC layout) instead of its fp16 weight argument; sdeo_debug_gemm_multi_f16 and the
 * block-scaled entries drop it unused.  Every one of them disarms first, so a refused call leaves nothing armed */
/* block-scaled fp8 (e4m3fn codes + one e8m0 scale per 32 elements of a row) at op level: the pack of an fp16 [rows][cols] matrix
 * (q_out [rows][cols] bytes, scales_out [rows][cols / 32] bytes) and y = x w^T on two packed operands with v_mfma_scale_f32_16x16x128_f8f6f4 */
int sdeo_debug_quantize_mx(void* q_out, void* scales_out, const void* x, int rows, int cols, void* stream);
int sdeo_debug_gemm_mx_f16(void* y, int ldy, const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* res,
                           int ldres, int m, int n, int k, int act, void* workspace, size_t workspace_bytes, void* stream);
/* gemm_mx_ex: sdeo_debug_gemm_mx_f16 with an output scale (ahead of the residual), a residual of res_rows rows (0: one per output
 *   row), per-row (sum, sumsq) partials out (stats != NULL; *strips_out = 0 with a split-K plan: the GEMM still runs, the statistics
 *   are sdeo_debug_row_stats_f16's) and a LayerNorm-folded input (ln_stats != NULL, as sdeo_debug_gemm_ln_f16 takes it); act 3 = the
 *   GEGLU pair on weights in geglu_interleave order (ldy >= n / 2) */
int sdeo_debug_gemm_mx_ex_f16(void* y, int ldy, const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* res,
                              int ldres, int res_rows, int m, int n, int k, int act, float scale, float* stats, int stats_ld, int* strips_out,
                              const float* ln_stats, const float* ln_s, int ln_ld, int ln_strips, int ln_c, float eps, void* workspace,
                              size_t workspace_bytes, void* stream);
int sdeo_debug_quantize_fp8_rows(void* w_f16_inout, void* q_out, float* scale_out, int rows, int cols, void* stream);
void sdeo_debug_next_weights_fp8(const void* q, const float* scale);

/* GEMM launches of the configured programs (ControlNet, UNet with and without control) that run on the block-scaled fp8 MFMA
 * (sdeo_set_activation_precision(h, 8, ...)) */
int sdeo_debug_mx_launches(sdeo_handle h);

/* one sdeo_fake_scribble_u8 call (same arguments) with HIP events between its three launches; synchronises and returns the JSON array
 * [{"kernel", "launches", "total_ms"}] (tools/scribble_time.py), "[]" when the call fails.  Not capturable. */
const char* sdeo_debug_fake_scribble_profile(const uint8_t* edges, int h, int w, uint8_t* scribble, float* control_chw, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* F.max_pool2d(x, 2, 2) on one NHWC fp16 image [h][w][c], c % 8 == 0 -> y [h / 2][w / 2][c] (csrc/hed.hip; tests) */
int sdeo_debug_maxpool2x2_f16(void* y, const void* x, int h, int w, int c, void* stream);
/* one HED detection with HIP events around every launch: the JSON array of sdeo_profile_end, "[]" on failure (tools/hed_time.py) */
const char* sdeo_debug_hed_profile(sdeo_hed_handle h, const uint8_t* img_hwc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDEO_INTERNAL_H */
