// Host-side launchers of the hand-written gfx950 kernels.  All are asynchronous on `stream`,
// never allocate and never synchronise (hipGraph-capturable).
#pragma once
#include <vector>

#include "common.h"

namespace sdeo {

// ------------------------------------------------------------------------------------------
// Implicit-GEMM convolution / GEMM on MFMA:   Y[M][N] = epi( sum_k A(m,k) * W[n][k] )
//   A(m,k) is gathered on the fly from an NHWC fp16 tensor (im2col never materialised):
//   m -> (b, ho, wo), k -> (r, s, c);  R=S=1 gives a plain row-major GEMM (Linear / conv1x1).
//   W is K-contiguous: [N][R][S][Cin] (KRSC) == nn.Linear's native [out][in].
//   epilogue:  v = acc + bias[n] + bias2[b][n];  v = act(v);  v = v*scale + res[m][n]
// ------------------------------------------------------------------------------------------
struct ConvGemm {
  const f16* x = nullptr;      // activations, pixel stride ldx elements
  const f16* w = nullptr;      // weights [N][K], row stride ldw
  f16* y = nullptr;            // fp16 output (row stride ldy) ...
  float* y32 = nullptr;        // ... or fp32 output when set
  const float* bias = nullptr;   // [N]   (or [M] when bias_per_row)
  const float* bias2 = nullptr;  // [B][ld_bias2], indexed by the batch of row m (time-embedding add)
  const f16* res = nullptr;      // residual [M][ldres]
  float* workspace = nullptr;    // split-K partials, >= splitk*M*N floats
  size_t workspace_bytes = 0;
  int M = 0, N = 0, K = 0;
  int B = 1, Hi = 1, Wi = 1, Cin = 0;  // source tensor geometry (Cin = channels consumed per tap)
  int Ho = 1, Wo = 1, R = 1, S = 1, stride = 1, pad = 0;
  int pad_after = -1;          // zero padding at the bottom / right (`pad` is the top / left one); -1: = pad.  The VAE encoder's
                               // Downsample is F.pad(x, (0,1,0,1)) + conv3x3 stride 2 pad 0 = pad 0, pad_after 1 (model.py:78-86)
  int ups = 0;                 // 1: the conv sees the source nearest-upsampled x2 (Upsample folded in)
  int ldx = 0, ldw = 0, ldy = 0, ldres = 0, ld_bias2 = 0;
  int act = 0;                 // 0 none, 1 SiLU, 2 quick-GELU  v * sigmoid(1.702 v)  (CLIP MLP),
                               // 3 GEGLU pair: W rows interleaved value/gate in blocks of 16, y gets N/2 columns v * gelu(g)
                               // 4 ReLU (HED's VGG stack); plans like act 0 (not part of the plan key)
                               // 5 erf GELU (the OpenCLIP text tower's MLP); plans like act 0, never with bias2
  int bias_per_row = 0;
  float scale = 1.0f;
  int force_tile = -1;         // testing hook: tile config index
  int force_splitk = 0;
  // LayerNorm folded into the GEMM (see KP::ln_stats in conv_inl.h): x is used raw, w = W * gamma, bias = b + W beta,
  // ln_s[n] = sum_k w[n][k]; ln_stats = the per-row partial (sum, sumsq) the producer of x emitted (ln_strips valid of ln_ld)
  const float* ln_stats = nullptr;
  const float* ln_s = nullptr;
  int ln_strips = 0, ln_ld = 0;
  int ln_c = 0;                // channels normalised over (= K for rows mode)
  float ln_eps = 1e-5f;
  // fp8 weights (OCP e4m3fn): `w` points at [N][K] BYTES (ldw in bytes), wscale[N] = per-output-channel scale (a power of two:
  // the product is then bit-identical to the fp16 kernel run on the dequantised weights).  Implicit-GEMM DMA kernel only.
  const float* wscale = nullptr;
  // emit per-row partial (sum, sumsq) of the stored fp16 values: stats_out[m][stats_ld][2], conv_gemm_stats_strips(p) valid
  float* stats_out = nullptr;
  int stats_ld = 0;
  // emit GroupNorm partials of the stored fp16 values: gn_out[b][gn_slots][gn_groups][2] = (sum, sumsq) of the gn_cpg channels of a
  // group over the rows of one M tile of image b; gn_slots must equal conv_gemm_gn_slots(p, gn_cpg) (> 0)
  float* gn_out = nullptr;
  int gn_cpg = 0, gn_slots = 0, gn_groups = 0;
  // block-scaled fp8 GEMM (both operands OCP e4m3fn codes + one e8m0 scale byte per 32 codes of a row, quantize_mx): x and w point at
  // BYTES, K / ldx / ldw count codes, K % 128 == 0, R = S = 1.  Runs on v_mfma_scale_f32_16x16x128_f8f6f4.
  const uint8_t* mx_sx = nullptr;  // [M][mx_ldsx]
  const uint8_t* mx_sw = nullptr;  // [N][mx_ldsw]
  int mx_ldsx = 0, mx_ldsw = 0;
  // shared prefix of a batch whose halves are identical up to here (the CFG pair, csrc/net_build.hip build_attn):
  // res_rows: `res` holds this many rows and output row m adds row m - res_rows when m >= res_rows (0: M rows, one per output row;
  //   M / 2: both halves of the batch add the residual the first half computed).  M / 2 <= res_rows <= M.
  // plan_B: this launch is the first B images (rows, for a GEMM) of a problem of plan_B; it runs that problem's plan (tile, split-K,
  //   K-steps), so every output row is computed by the instruction sequence it has in the full-batch launch.  0: its own plan.
  int res_rows = 0;
  int plan_B = 0;
};
int conv_gemm(const ConvGemm& p, hipStream_t stream);
inline int conv_pad_after(const ConvGemm& p) { return p.pad_after < 0 ? p.pad : p.pad_after; }
// Multi-problem launch: up to kMultiMax conv / GEMM problems that run on ONE tile of the table, unsplit, as one grid of the
// LDS-DMA kernel (the sum of their tiles): thirteen 10 us launches become one many-tile launch.  fp16 weights, Cin % 64 == 0, no
// folded Upsample, no statistics / GroupNorm-partial / LayerNorm-fold epilogue; bias, bias2, residual, act (not the GEGLU pair), scale and
// output views behave as in conv_gemm(), and every problem's output is bit-identical to its own launch with that tile forced.
//   conv_gemm_multi_plan: host only, no device call.  tile: a row of the table that has a multi-problem instantiation (< 0: the
//     problems' own force_tile, which must then agree); a problem whose force_tile names another row is refused ("mixed tiles"), as is
//     a force_splitk above 1 (the process-wide conv_gemm_debug_force does not reach these launches).  Fills `out`: table = the image of the device table the launch reads.
//   conv_gemm_multi_launch: table_dev = out.table copied to device memory (16-byte aligned), by the caller, once; scales[count] = the
//     problems' `scale` at the moment of the launch (null: those of the plan).
constexpr int kMultiMax = 16;
struct ConvGemmMultiPlan {
  int tile = -1, count = 0, tiles = 0;
  std::vector<char> table;
  float scale[kMultiMax] = {};
  double flops = 0, bytes = 0;     // sums over the problems (2 M N K; algorithmic bytes of x, w, y)
  const char* name = "";           // the tile's instantiation
};
int conv_gemm_multi_plan(const std::vector<ConvGemm>& ps, int tile, ConvGemmMultiPlan* out);
int conv_gemm_multi_launch(const ConvGemmMultiPlan& pl, const void* table_dev, const float* scales, hipStream_t stream);
// The live-row form of the same launch (its own kernel instantiation; the zero convs' tile has one): problem i computes its first
// m_live[i] rows (0..M) and every row beyond them receives its `res` row unchanged -- selected, not scaled, so what x holds there never
// matters; nothing is written there when res is the output itself or null.  Row tiles wholly beyond m_live run no K loop.  The live
// rows are bit-identical to conv_gemm_multi_launch's.  Needs fp16 outputs, one residual row per output row, N / ldy / ldres % 4 == 0.
int conv_gemm_multi_launch_live(const ConvGemmMultiPlan& pl, const void* table_dev, const float* scales, const int* m_live, hipStream_t stream);
// M tiles per image of the plan chosen for p when its epilogue can emit GroupNorm partials for groups of cpg channels, else 0
int conv_gemm_gn_slots(const ConvGemm& p, int cpg);
// whether the plan chosen for p is a halo-reuse 3x3 kernel (which has no fp8-weight variant)
bool conv_gemm_plan_is_halo(const ConvGemm& p);
// strips (partials per row) a launch of p writes to stats_out; 0 when the chosen plan cannot emit them (split-K)
int conv_gemm_stats_strips(const ConvGemm& p);
// measurement only: phase stamps of the last launch of an implicit-GEMM / halo kernel (SDEO_DBG_GEMM bit 6), see conv_inl.h
int conv_gemm_read_stamps(unsigned long long* out, int n);
int conv_halo_read_stamps(unsigned long long* out, int n);
size_t conv_gemm_workspace_bytes(const ConvGemm& p);
int conv_gemm_plan_splitk(const ConvGemm& p);       // split-K factor of the plan chosen for p
// tests: the tuned-table key of p and the (tile, split-K) the launcher picks for it (host only); the plan of the last launch
void conv_gemm_query_plan(const ConvGemm& p, int key[10], int* tile, int* splitk);
void conv_gemm_last_plan(int* tile, int* splitk);
int conv_gemm_last_epilogue();                     // 0 the staged family, 1 EPI_DIRECT
int conv_gemm_last_epilogue_mode();                // the EpiKind within the staged family (conv_inl.h), 0 = the generic kernel
void conv_gemm_debug_force_epilogue_mode(int mode);      // -1 automatic, 0 every non-direct launch on the generic kernel
int conv_gemm_tile_has_epilogue_mode(int tile, int mode);
// launches dispatched since the last clear as rows of (tile, split-K, operand form, EpiKind, mode flags, count): conv_gemm.hip, g_census
int conv_gemm_epilogue_census(int* rows6, int cap, int clear);
// row `tile` of the tile table (kind: TileKind, caps: TileCap bits, conv_inl.h); non-zero past the end
int conv_gemm_tile_info(int tile, int* kind, int* bm, int* bn, int* stages, int* caps, const char** name);
// name of the kernel instantiation the launcher will pick (for profiles; matches the rocprof kernel name's template args)
const char* conv_gemm_kernel_name(const ConvGemm& p);
void conv_gemm_debug_force(int tile, int splitk);
void conv_gemm_debug_force_order(int order);       // -1 heuristic, 0 M-fastest, 1 N-fastest tile order
// one-time on-device plan search for p's shape (p needs valid scratch pointers); workspace to reserve for it
int conv_gemm_autotune(const ConvGemm& p, hipStream_t stream);
size_t conv_gemm_autotune_workspace_bytes(const ConvGemm& p);
void conv_gemm_set_tuned(const int key[10], int tile, int splitk);
std::string conv_gemm_tuned_json();   // [[M,N,K,Cin,R,stride,ups,Hi,Wi,B,tile,splitk],...]   // tuning hook: -1 / 0 restore the heuristic

// ------------------------------------------------------------------------------------------
// GroupNorm (NHWC fp16, fp32 statistics, eps honoured) + optional SiLU; two launches:
// per-chunk partial sums, then normalise.  `partials` >= B*gn_chunks(HW)*groups*2 floats.
// ------------------------------------------------------------------------------------------
int gn_chunks(int HW);
int groupnorm_nhwc(f16* y, int ldy, const f16* x, int ldx, const float* gamma, const float* beta, int B, int HW, int C,
                   int groups, float eps, int with_silu, float* partials, hipStream_t stream);

struct GnArgs {
  f16* y; const f16* x; const float* gamma; const float* beta; float* partials;
  int ldy, ldx, B, HW, C, groups;
  float eps;
  int with_silu;
  // statistics already exist: ext_partials[b][ext_nsc][groups][2] = (sum, sumsq) partials written by the epilogue of the conv / GEMM
  // that produced x (ConvGemm::gn_out).  Then no statistics pass runs: ONE launch normalises (plus a small reduction launch when
  // ext_nsc > 128, the VAE's large images: `partials` is its workspace, >= B * groups * 2 floats)
  const float* ext_partials = nullptr;
  int ext_nsc = 0;
};
// whether groupnorm_nhwc(a) runs as ONE launch with its slice in LDS
bool groupnorm_is_single_launch(const GnArgs& a);
// the launcher's own selection for a (only HW, C and groups are read; C % groups == 0): 0 = two launches (statistics, apply),
// 256 / 1024 = threads of the single-launch kernel.  Host only.
int gn_fused_threads(const GnArgs& a);
int groupnorm_nhwc(const GnArgs& a, hipStream_t stream);

// LayerNorm over the last dim of [rows][C] fp16 (two-pass in registers, fp32 math).
int layernorm(f16* y, int ldy, const f16* x, int ldx, const float* gamma, const float* beta, int rows, int C, float eps,
              hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Fused attention  O = softmax(Q K^T * scale) V   (flash-style, scores never materialised)
//   Q[(b*Tq+t)*ldq + h*d + i], K[(b*TkS+j)*ldk + h*d + i], V[(b*TkSv+j)*ldv + h*d + i]   (all row-major)
//   O[(b*Tq+t)*ldo + h*d + i];  keys j >= Tk are masked;  TkS / TkSv = per-batch row strides of K / V.
//   causal: key j additionally masked for query t when j > t (needs Tq == Tk).
// ------------------------------------------------------------------------------------------
int attention(f16* o, int ldo, const f16* q, int ldq, const f16* k, int ldk, const f16* v, int ldv, int B, int H,
              int Tq, int Tk, int TkS, int TkSv, int d, float scale, hipStream_t stream, int causal = 0);
struct AttnArgs {
  f16* o; const f16* q; const f16* k; const f16* v;
  int ldo, ldq, ldk, ldv, B, H, Tq, Tk, TkS, TkSv, d;
  float scale;
  int causal;
  // shared prefix of a batch whose halves are identical up to here (the CFG pair, csrc/net_build.hip build_attn):
  // qB: batches of Q; batch b reads the queries of batch b - qB when b >= qB (0: B, one per batch; B / 2 <= qB <= B)
  // plan_B: select the kernel as for a problem of plan_B batches (this launch is a batch prefix of it); 0: B
  int qB = 0;
  int plan_B = 0;
};
int attention(const AttnArgs& a, hipStream_t stream);
// the instantiation attention() launches for this shape ("attention_kernel<3,2,true,4>", "attention_wide_kernel<128>"), from the
// launcher's own selection; nullptr with the error set for a shape attention() rejects.  Host only.
const char* attention_kernel_name(int B, int H, int Tq, int Tk, int d, int causal);
// Two key segments, two softmaxes, ONE launch:  O = softmax(Q K^T * scale) V + w * softmax(Q K2^T * scale) V2  (decoupled
// cross-attention: text keys, then the image-prompt keys).  a: the first segment exactly as attention() takes it (not causal; qB and
// plan_B included).  s2: K2[(b*TkS+j)*ldk + h*d + i], V2[(b*TkSv+j)*ldv + h*d + i], 1 <= Tk <= 64 keys, keys >= Tk masked.  Both
// normalised outputs and their sum stay in fp32; the result is rounded to fp16 once.  Head dims of the KS = 1 kernels (8..160).
struct Attn2Seg {
  const f16* k; const f16* v;
  int ldk, ldv, Tk, TkS, TkSv;
  float w;
};
int attention2(const AttnArgs& a, const Attn2Seg& s2, hipStream_t stream);
// the checks attention2() makes before its launch, alone: 0, or the refusal.  Host only, never touches an operand.
int attention2_check(const AttnArgs& a, const Attn2Seg& s2);
// the instantiation attention2() launches ("attention2_kernel<3,true>": D16, MPAD); nullptr with the error set for a rejected shape
const char* attention2_kernel_name(int B, int H, int Tq, int Tk, int Tk2, int d);
// vt[c][b*TkSv + t] = v[(b*T + t)*ldv + c]   (VAE AttnBlock's materialised-score path)
int transpose_pad(f16* vt, int ldvt, const f16* v, int ldv, int B, int T, int TkSv, int C, hipStream_t stream);

// row softmax: fp32 scores [rows][ld] -> fp16 probabilities (VAE single-head attention)
int softmax_rows(f16* p, int ldp, const float* s, int lds, int rows, int cols, float scale, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// elementwise / layout kernels
// ------------------------------------------------------------------------------------------
// y[m][0:C] = a[m][0:C] * gelu(a[m][C:2C])      (GEGLU, exact erf GELU)
int geglu(f16* y, int ldy, const f16* a, int lda, int rows, int C, hipStream_t stream);
// y = a + b*scale (b may be null), fp16, strided rows of C channels
int add_scaled(f16* y, int ldy, const f16* a, int lda, const f16* b, int ldb, float scale, int rows, int C,
               hipStream_t stream);
// sinusoidal timestep embedding (util.py:154-174): out[b][dim] fp16
int timestep_embedding(f16* out, const int64_t* t, int B, int dim, hipStream_t stream);
int silu(f16* y, const f16* x, int64_t n, hipStream_t stream);
// layout / dtype conversion at the NCHW boundary
int nchw_f32_to_nhwc_f16(f16* y, int ldy, const float* x, int B, int C, int HW, float scale, hipStream_t stream);
// context [B][T][C] fp32 -> fp16 [B][Tpad][C], rows >= T zero
int pad_rows_f32_to_f16(f16* y, const float* x, int B, int T, int Tpad, int C, hipStream_t stream);
int nhwc_f16_to_nchw_f32(float* y, const f16* x, int ldx, int B, int C, int HW, float scale, hipStream_t stream);
// VAE encoder intake: images fp32 NCHW [B][C][HW] in [-1,1] OR (x == nullptr) uint8 HWC [B][HW][C] mapped as 2 * (u / 255.0f) - 1 in
// fp32 -> fp16 NHWC [B][HW][8] (C <= 8 channels, the stored ones above C zero)
int image_to_nhwc8_f16(f16* y, const float* x, const uint8_t* x_u8, int B, int C, int HW, hipStream_t stream);
// DiagonalGaussianDistribution of the VAE encoder's moments (distributions.py:24-35 + get_first_stage_encoding) on one image:
// m fp16 NHWC [HW][ldm], channels [0, zc) = mean, [zc, 2zc) = logvar.  moments fp32 NCHW [2zc][HW] (may be null) = m as stored;
// z fp32 NCHW [zc][HW] = scale * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise), or scale * mean when noise is null
int vae_posterior(float* z, float* moments, const f16* m, int ldm, const float* noise, int zc, int HW, float scale, hipStream_t stream);
int nhwc_f16_to_nhwc_u8(uint8_t* y, const f16* x, int ldx, int64_t pixels, int C, hipStream_t stream);
// weights: fp32 [O][I][R][S] -> fp16 [O][R][S][Ipad]
int oihw_f32_to_ohwi_f16(f16* y, const float* w, int O, int I, int R, int S, int Ipad, hipStream_t stream);
int zero_f16(f16* y, int64_t n, hipStream_t stream);
int f32_to_f16(f16* y, const float* x, int64_t n, hipStream_t stream);
int f16_to_f32(float* y, const f16* x, int64_t n, hipStream_t stream);
// GEGLU projection [2H][cols] fp32 -> fp16 with value / gate rows interleaved in blocks of 16 (see conv_gemm act = 3); bias variant
int geglu_interleave_f32_to_f16(f16* y, const float* x, int H, int cols, hipStream_t stream);
int geglu_interleave_f32(float* y, const float* x, int H, hipStream_t stream);
// LoRA merge into a stored tensor (csrc/lora.hip): w[o][j] <- fp16(fp32(w[o][j]) + scale * sum_r up[o][r] down[r][j]) with (o, j)
// where WeightStore::load put it.  kind: the tensor's WKind (W_LINEAR, W_CONV or W_GEGLU_W); out / in / k / ipad its logical shape
// ([out][in][k][k], k = 1 for a matrix) and stored input channels; down [rank][in * k * k], up [out][rank]: fp32 DEVICE pointers.
int lora_merge_f16(f16* w, int kind, int out, int in, int k, int ipad, const float* down, const float* up, int rank, float scale,
                   hipStream_t stream);
// LoHa / LoKr merge into a stored tensor (csrc/lora.hip; include/sdeo.h: sdeo_loha_merge_f16 / sdeo_lokr_merge_f16 define the forms).
// The operands of one module as the file holds them, fp32, HOST OR DEVICE pointers, absent ones null:
//   LoHa: a1 / b1 / t1 = hada_w1_a / hada_w1_b / hada_t1, a2 / b2 / t2 likewise, rank1 the rank of both
//   LoKr: w1 or a1 @ b1 (rank1);  w2 or a2 @ b2 or the Tucker form t2, a2, b2 (rank2);  out_l x in_m the shape of w1
struct LycoOps {
  int algo = 0;                      // LYCO_LOHA, LYCO_LOKR
  const float *w1 = nullptr, *a1 = nullptr, *b1 = nullptr, *t1 = nullptr;
  const float *w2 = nullptr, *a2 = nullptr, *b2 = nullptr, *t2 = nullptr;
  int rank1 = 0, rank2 = 0;
  int out_l = 0, in_m = 0;
};
enum { LYCO_LOHA = 1, LYCO_LOKR = 2 };
// every refusal that depends on the operands and the tensor's shape, no device call: a missing or mixed operand set, a rank outside
// 1..1024, factor shapes that do not fit [out][in][k][k] (a Tucker core on a matrix included)
int lyco_check(const char* who, const LycoOps& ops, int kind, int out, int in, int k);
// floats of staging the merge needs (the operands as given + the composed ones of the pre-pass)
size_t lyco_stage_floats(const LycoOps& ops, int out, int in, int k);
// copies the operands into `stage` (a device buffer of lyco_stage_floats), runs the pre-pass and the merge on `stream`; the caller has
// run lyco_check and synchronises before it reuses the buffer
int lyco_merge_f16(f16* w, int kind, int out, int in, int k, int ipad, const LycoOps& ops, float* stage, float scale, hipStream_t stream);
// the inverse of WeightStore::load for the same kinds: out_f32 [out][in][k][k] = fp32 of the stored values, pad channels dropped
int lora_read_f32(float* out_f32, const f16* w, int kind, int out, int in, int k, int ipad, hipStream_t stream);
// LayerNorm folded into a Linear (KP::ln_stats): w_out = fp16(w * gamma), s = row sums of w_out, b_out = bias + w beta
int fold_layernorm(f16* w_out, float* s_out, float* b_out, const f16* w, const float* gamma, const float* beta,
                   const float* bias, int rows, int C, hipStream_t stream);
// stats[r][ld][2] <- one (sum, sumsq) partial per row of x [rows][C]
int row_stats(float* stats, int ld, const f16* x, int ldx, int rows, int C, hipStream_t stream);
// fp8 weight pack: q[r][0:cols] = e4m3fn codes of w[r] / scale[r] (scale = power of two, absmax / scale <= 448) and w <- code * scale
int quantize_fp8_rows(uint8_t* q, float* scale, f16* w, int rows, int cols, int ldw, int ldq, hipStream_t stream);
int row_sums_f16(float* s_out, const f16* w, int rows, int C, hipStream_t stream);
// [ (Wp W2) | Wp ] and Wp b2 + bp: ff.net.2 and proj_out of a SpatialTransformer as one Linear over [g | t] (elementwise.hip)
int compose_proj(f16* w_out, float* b_out, const f16* wp, const float* bp, const f16* w2, const float* b2, int C, int K2,
                 hipStream_t stream);
// block-scaled fp8 pack of a [rows][cols] fp16 matrix (cols % 32 == 0): per 32 consecutive elements of a row one e8m0 scale byte
// (2^(s - 127): the smallest power of two with amax / scale <= 448; 127 for an all-zero block) and 32 e4m3fn codes of x / scale
int quantize_mx(uint8_t* q, uint8_t* scales, const f16* x, int rows, int cols, int ldx, int ldq, int lds, hipStream_t stream);
// CLIP text embeddings: out[(b*T + t)][0:W] = tok_emb[ids[b*T + t]][0:W] + pos_emb[t][0:W]   (ids are clamped to [0, vocab))
int embed_tokens(f16* out, const int32_t* ids, const f16* tok_emb, const f16* pos_emb, int B, int T, int W, int vocab,
                 hipStream_t stream);
// cv2.Canny(img, low, high) (aperture 3, L1 magnitude) on an HWC uint8 image of 1..4 channels -> edges [H][W] uint8 0 / 255 and / or
// control [3][H][W] fp32 = edges / 255.  Asynchronous, capturable (hysteresis = union-find labelling).  csrc/canny.hip
size_t canny_workspace_bytes(int H, int W);
int canny_u8(const uint8_t* img, int H, int W, int C, float low_threshold, float high_threshold, uint8_t* edges, float* control,
             void* workspace, size_t workspace_bytes, hipStream_t stream);
// cv2.resize on 8-bit HWC images (csrc/resize.hip); the coefficient tables are built on the host (annotator/util.py)
int resize_lanczos4_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dh, int dw, const int* x0, const short* ax,
                       const int* y0, const short* by, hipStream_t stream);
int resize_area_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dh, int dw, const int* xstart, const int* xidx,
                   const float* xw, const int* ystart, const int* yidx, const float* yw, hipStream_t stream);
int resize_area_fast_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dh, int dw, hipStream_t stream);
// classifier-free guidance + DDIM update on NCHW fp32 latents (ddim_hacked.py:192,208-231).  The pair form takes the UNet's fp16 NHWC
// output, updates x in place and stages the fp16 NHWC latent of the next forward in both halves of x0.  noise (fp32, laid out like x) set:
// + sigma_t * noise with dir_coef = sqrt(1 - a_prev - sigma_t^2) (`cldm/ddim_hacked.py:227-230`), one more fused multiply-add, bit-equal
// to cfg_ddim_step with the same noise / sigma_t, and the staged latent is the noisy one; noise null: sigma_t is not read.
// paired = false (every pair launcher here): the un-paired member, SDEO_STEP_UNGUIDED.  b is the whole batch, eps rows 0..b-1 are used as
// they are (cfg_scale is not read), and each image is staged once: bit-equal to the flat step with a null eps_u / m_u.
int cfg_ddim_pair(float* x, float* pred_x0, const f16* eps, int lde, const float* noise, float sigma_t, f16* x0, int ld0, int b, int C, int HW,
                  float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at, bool v_prediction, bool paired, hipStream_t stream);
int latent_pair_to_nhwc(f16* x0, int ld0, const float* x, int b, int C, int HW, bool paired, hipStream_t stream);
int cfg_ddim_step(float* x_prev, float* pred_x0, const float* x, const float* eps_c, const float* eps_u, const float* noise,
                  float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, int64_t n,
                  bool v_prediction, hipStream_t stream);
// classifier-free guidance + one linear-multistep update x_next = k_x x + k_d D + k_p D_prev + k_n noise (DPM-Solver++(2M) and its SDE
// form); D is cfg_ddim_step's pred_x0 and replaces D_prev in d.  k_n == 0 is the deterministic update, whatever the noise pointer (it may
// be null).  The pair form is laid out as cfg_ddim_pair.  `who` names the flat step in its refusals.
int cfg_lms_pair(float* x, float* d, const f16* eps, int lde, const float* noise, float k_n, f16* x0, int ld0, int b, int C, int HW,
                 float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, bool v_prediction, bool paired,
                 hipStream_t stream);
int cfg_lms_step(const char* who, float* x_next, float* d, const float* x, const float* m_c, const float* m_u, const float* noise,
                 float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n, int64_t n, bool v_prediction,
                 hipStream_t stream);
// host-side checks of the two pair updates (no device call), for callers that must refuse before they launch anything.  sigma_t null:
// the deterministic DDIM update (noise is not looked at); k_n = 0: the deterministic multistep update.
int cfg_ddim_check(const char* who, float a_t, float a_prev, const float* noise, const float* sigma_t);
int cfg_lms_check(const char* who, const float* d, const float* noise, float a_t, float k_x, float k_d, float k_p, float k_n);
// The sampler's mask / x0 blend (cldm/ddim_hacked.py:154-157) on fp32 NCHW latents [n][C][HW], in place:
//   x <- mask * (sqrt_a * orig + sqrt_1ma * noise) + (1 - mask) * x,   mask [mask_n][mask_c][HW], mask_n in {1, n}, mask_c in {1, C}
// rounded operation by operation like the torch expression (no fma contraction).  mask_blend_pair: the same blend as the front of a fused
// CFG-pair step, in the layout of latent_pair_to_nhwc, whose place it takes: the fp16 NHWC copy of the blended latent goes to both halves
// of x0 (padding channels zero).  mask_blend_check: their operand checks alone (host only).
int mask_blend_check(const char* who, const float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c,
                     int n, int C, int HW);
int mask_blend(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a, float sqrt_1ma,
               int n, int C, int HW, hipStream_t stream);
int mask_blend_pair(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a,
                    float sqrt_1ma, f16* x0, int ld0, int b, int C, int HW, bool paired, hipStream_t stream);
// dst = (gen * m + orig * (255 - m) + 127) / 255 in integers: uint8 HWC images [H][W][C], C in 1..4, uint8 mask [H][W]
int composite_u8(uint8_t* dst, const uint8_t* gen, const uint8_t* orig, const uint8_t* mask, int H, int W, int C, hipStream_t stream);

// FreeU on one decoder concat buffer, in place (freeu.hip; include/sdeo.h: sdeo_freeu_nhwc_f16 defines the arithmetic).  buf: fp16 NHWC
// [n * h * w][ld], h in columns [0, c_h), the skip in [c_h, c_h + c_skip); nothing else is touched.  version 1: one launch; version 2:
// the mean-map launch into `workspace` (freeu_workspace_bytes: n * h * w floats), then the apply launch.  b == 1 / s == 1 launch nothing
// for their half.  No allocation, no synchronisation.  freeu_check: the operand checks alone; freeu_params_check: the four values and
// the version as sdeo_set_freeu takes them (both host only).
constexpr float kFreeuMax = 8.0f;      // cap of b and s: b times an fp16 activation of up to 65504 / 8 = 8188 stays finite
constexpr int kFreeuMaxDim = 512;      // largest map height / width (the trigonometric tables of a skip workgroup live in LDS)
int freeu_params_check(const char* who, float b1, float b2, float s1, float s2, int version);
int freeu_check(const char* who, const f16* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version,
                const float* workspace);
size_t freeu_workspace_bytes(int n, int h, int w);
int freeu_nhwc_f16(f16* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version, float* workspace,
                   hipStream_t stream);

}  // namespace sdeo
