/* libomp355 -- MI355X (gfx950) kernels for the OmniParser inference hot path.
 *
 * C ABI.  The reference (AlibabaResearch/AdvancedLiterateMachinery, OCR/OmniParser) has no
 * FFI/plugin layer: its hot path is plain nn.Module composition on ATen ops.  Each entry point
 * below therefore names the reference *function* it replaces (paths relative to
 * OCR/OmniParser/).  INTEGRATION.md shows the ctypes stub a maintainer would drop into the
 * reference for each of them.
 *
 * Rules of the ABI
 *   - every function returns 0 on success or a negative errno-style code; omp_last_error()
 *     returns a thread-local description of the last failure;
 *   - the CALLER owns every buffer (device pointers); the library never allocates device
 *     memory, never synchronises the device and launches only on the given stream
 *     (hipStream_t passed as void*; NULL = the null stream);
 *   - matrices are row-major; activations are token-major [rows, channels];
 *     weights keep the reference's nn.Linear layout [out_features, in_features];
 *   - dtype enum: OMP_F32 / OMP_BF16 for activations+weights; biases, LayerNorm affine
 *     parameters, embedding and bias tables are always fp32; accumulation is fp32.
 *   - development hooks (kernel selectors, trace buffers, measurement brackets, CU-masked streams) are declared in
 *     csrc/omp355_debug.h, not here: they are exported for the tests and tools of this repository only.
 */
#ifndef OMP355_H
#define OMP355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMP_ABI_VERSION 24
#define OMP_MAX_DEC_LAYERS 8

enum { OMP_OK = 0, OMP_ERR_LAUNCH = -5, OMP_ERR_INVALID = -22, OMP_ERR_UNSUPPORTED = -95 };
/* OMP_BF16X2 = split-bf16 pair rows: a [rows, C] tensor is stored as rows of 2C bf16, hi = bf16(x) in columns 0..C-1 and
 * lo = bf16(x - hi) in columns C..2C-1 (16 mantissa bits, the same bytes as fp32).  It is the GEMM-operand format of the
 * bf16x3 engine: x.w ~ hi.w_hi + lo.w_hi + hi.w_lo on the bf16 matrix cores (see omp_gemm_args.a_wrap). */
enum { OMP_F32 = 0, OMP_BF16 = 1, OMP_BF16X2 = 2 };
enum { OMP_ACT_NONE = 0, OMP_ACT_GELU = 1, OMP_ACT_RELU = 2 };
enum { OMP_STORE_PLAIN = 0, OMP_STORE_KBLK = 2, OMP_STORE_VBLK = 3, OMP_STORE_ROWSTAT = 4 };
/* decoder kinds (reference: model/transformer.py:26-33 pt/poly/rec decoders) */
enum { OMP_DEC_PT = 0, OMP_DEC_POLY = 1, OMP_DEC_REC = 2 };

typedef void* omp_stream_t; /* hipStream_t */

const char* omp_last_error(void);
int omp_abi_version(void);

/* ---- LayerNorm ---------------------------------------------------------------------------
 * y = (x - mean) / sqrt(var + eps) * gamma + beta over the last dim (biased variance).
 * Replaces nn.LayerNorm call sites: swin_transformer.py:208,250,288,441,616 and
 * transformer.py:326,374,437,441,450.  Writes y (dtype y_dtype, may be NULL; OMP_BF16X2 = split pairs [rows, 2C]) and/or y_f32. */
int omp_layernorm(const void* x, int x_dtype, const float* gamma, const float* beta, void* y,
                  int y_dtype, float* y_f32, int64_t rows, int C, float eps, omp_stream_t s);

/* omp_layernorm of the pixels the FPN neck reads (omp_fpn_fuse_sampled): x is a token-major [B, H, W, C] map, y (OMP_F32 or
 * OMP_BF16) the compact [B, H / step * group, W / step * group, C] map of the rows and columns q * step + r, r < group, in order;
 * no other pixel of x is read.  H and W multiples of step, 1 <= group <= step.  A row's result is omp_layernorm's, bit for bit. */
int omp_layernorm_sampled(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, int B, int H,
                          int W, int C, int step, int group, float eps, omp_stream_t s);

/* ---- GEMM with fused epilogue ---------------------------------------------------------------
 * C[m,n] = act(sum_k A[m,k] * W[n,k] + bias[n]) + residual[m,n]
 * Replaces nn.Linear / 1x1 nn.Conv2d call sites: swin_transformer.py:127,148 (qkv, proj),
 * :31-34 (Mlp fc1+GELU, fc2), :294 (PatchMerging.reduction), fpn.py:24-36 (fpn_in 1x1 convs),
 * omniparser.py:31 (input_proj), transformer.py:448 (linear1/2) and the in/out projections of
 * nn.MultiheadAttention (transformer.py:386-387), block/mlp.py:11-13 (prediction heads).
 * bias_row (device int32, optional) selects row *bias_row of a [rows, bias_row_stride] bias table
 * (used for the per-position query/key bias of the decoders).  bias_row_mod > 0 is the table's PER-ROW form:
 * row m takes table row (bias_row_off + m) % bias_row_mod and bias_row is not read (the batched prompt prefill of
 * omp_decoder_run, whose row r * L + j sits at position j).
 * trans_out: store C transposed per batch of `trans_rows` consecutive rows:
 *   C[(m / trans_rows) * N * trans_ld + n * trans_ld + (m % trans_rows)]   (ldc ignored). */
typedef struct {
  const void* A;
  int64_t lda;
  const void* W;
  int64_t ldw;
  const float* bias;
  const int32_t* bias_row;
  int64_t bias_row_stride;
  const void* residual;
  int64_t ldr;
  void* C;
  int64_t ldc;
  int64_t M;
  int32_t N;
  int32_t K;
  int32_t dtype;     /* of A and W */
  int32_t out_dtype; /* of C and residual: dtype, OMP_F32, or OMP_BF16X2 (dtype OMP_BF16, no residual: C is [M, 2N] split pairs) */
  int32_t act;
  int32_t trans_out;
  int64_t trans_rows; /* rows (tokens) per batch item */
  int64_t trans_ld;   /* pitch of a transposed row, >= trans_rows */
  /* optional fused LayerNorm prologue (decoder steps, M <= 64): A is then the fp32 residual stream
   * [M,K] and the GEMM consumes LN(A) * ln_gamma + ln_beta (transformer.py:437,441,450 + the Linear) */
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  int32_t small_m_splitk; /* hint: M <= 64 weight-streaming GEMM -> split-K workgroups */
  /* destination layout.  OMP_STORE_KBLK / OMP_STORE_VBLK write the decoder cross-attention memory
   * K / V straight into the head-blocked slabs omp_dec_cross_attn_step streams (see DESIGN.md
   * "cross-attention memory layout"):
   *   KBLK: M = kv_images*kv_tokens memory tokens, N = n_slabs*kv_heads*64 features ->
   *         C[slab][image][head][kv_mpad][64]
   *   VBLK: operands swapped by the caller (A = Wv [n_slabs*kv_heads*64, K], W = memory tokens
   *         [kv_images*kv_tokens, K], bias_along_m = 1) ->
   *         C[slab][image][head][kv_mpad/kv_key_block][64][kv_key_block], keys of a block in
   *         matrix-core order (bf16, block 32: slot 8g+4*half+r <- key 16*half+4g+r; f32, block 16: natural)
   *   with out_dtype OMP_BF16X2 (kv_key_block 32): SPLIT-PLANE slabs -- every 32-key block holds [hi plane | lo plane] of bf16,
   *         KBLK C[slab][image][head][kv_mpad/32][2][32][64], VBLK C[slab][image][head][kv_mpad/32][2][64][32] (the bytes of the
   *         fp32 slabs; read by omp_dec_cross_attn_step with dtype OMP_BF16X2) */
  int32_t store_mode;
  int32_t bias_along_m; /* bias[m] instead of bias[n] */
  int32_t kv_images, kv_tokens, kv_mpad, kv_heads, kv_key_block;
  /* optional second destination (plain row-major, pitch ldc2, same dtype as C): act(A W^T + bias) WITHOUT the residual.
   * One GEMM then yields both `memory` and `memory + pos` of omniparser.py:31 / transformer.py:88-96 (the reference
   * adds pos inside nn.MultiheadAttention's key path); requires a residual, OMP_STORE_PLAIN, no trans_out. */
  void* C2;
  int64_t ldc2;
  /* bf16x3 products (fp32-grade results at a third of the bf16 matrix-core rate; the parity engine):
   * A is a split-bf16 pair tensor [M, 2*K0] = [a_hi | a_lo] (OMP_BF16X2 rows, dtype stays OMP_BF16), W is the once-per-
   * checkpoint image [N, 3*K0] = [w_hi | w_hi | w_lo] of an fp32 weight, K = 3*K0 and a_wrap = 2*K0: A columns at and
   * beyond a_wrap are read from column (k - a_wrap), i.e. A is consumed as [a_hi | a_lo | a_hi] without being stored
   * that way.  The contraction is then a_hi.w_hi + a_lo.w_hi + a_hi.w_lo (the a_lo.w_lo term, 2^-16 relative, is
   * dropped).  With swapped operands (OMP_STORE_VBLK) the weight is the [hi | lo] side and the activation arrives as
   * [hi | hi | lo] (omp_split_bf16, triple = 1).  0 = plain product. */
  int32_t a_wrap;
  /* per-row form of the bias table (see above): plain row-major destinations without bias_along_m; honoured by the 64 x 64 and
   * 128 x 128 tile kernels and by the split-K small-M kernel, and the dispatch stays with them (a row's bits are the same on all
   * three tile sizes, so a row computed here equals the row a step computes with bias_row).  0 = off. */
  int32_t bias_row_mod, bias_row_off;
} omp_gemm_args;
int omp_gemm_bias_act(const omp_gemm_args* a, omp_stream_t s);

/* ---- Fused Swin MLP (bf16 engine):  y = x + fc2(GELU(fc1(LayerNorm(x)))) ---------------------------------------
 * Replaces `x = x + self.drop_path(self.mlp(self.norm2(x)))`, swin_transformer.py:250, with Mlp.forward (:30-36)
 * inlined: one launch, the [tokens, hidden] activation never reaches HBM.  x, y: bf16 [M, C] with row pitches
 * ldx / ldy (y may alias x); ln_gamma / ln_beta / b2 (= fc2.bias): fp32 [C]; wpack: fc1.weight, fc1.bias and
 * fc2.weight re-laid out once per checkpoint by model/packing.py::pack_mlp (hidden / 32 sub-chunk images of
 * C*128 + 1024 bytes; layout documented there and in csrc/mlp.hip).  C in {128, 256, 512}, hidden % 32 == 0. */
int omp_swin_mlp_fused(const void* x, int64_t ldx, const float* ln_gamma, const float* ln_beta, float eps,
                       const void* wpack, const float* b2, void* y, int64_t ldy, int64_t M, int C, int hidden,
                       omp_stream_t s);
/* the same with x / y of type x_dtype: OMP_BF16, or OMP_F32 = the fp32 residual stream of the bf16 engine (the products
 * still run on bf16 operands: LayerNorm(x) and the hidden activations are rounded to bf16, x itself never is) */
int omp_swin_mlp_fused2(const void* x, int x_dtype, int64_t ldx, const float* ln_gamma, const float* ln_beta, float eps,
                        const void* wpack, const float* b2, void* y, int64_t ldy, int64_t M, int C, int hidden,
                        omp_stream_t s);

/* ---- Swin-B stage 2 (C = 512, hidden 2048) as row-owner chains (round 5, csrc/dec_rows.hip) ------------------------------------------
 * Everything of a SwinTransformerBlock (swin_transformer.py:196-253) except the window attention core is row-local, so a block is the
 * window attention kernel (omp_swin_window_attn2 on bf16 q | k | v) plus ONE launch of this entry point:
 *   mode 0: qkv = bf16(LayerNorm(x; n1) Wqkv^T + bqkv)                                          (:208 + :127, the stage's first block)
 *   mode 1: x += att Wproj^T + bproj  (:148, :246);  x += fc2(GELU(fc1(LayerNorm(x; n2))))     (:250 with Mlp.forward :30-36 inlined);
 *           and, when n1_g != NULL, the NEXT block's qkv = bf16(LayerNorm(x; n1) Wqkv'^T + bqkv')
 * x: fp32 residual stream [M, 512], in place; att: bf16 [M, 512] (attention output in token order); qkv: bf16 [M, 1536].  A workgroup owns
 * omp_dec_rows_tile() tokens and streams the weights: wstream is written once per checkpoint by model/packing.py (pack_rows_embed_qkv for
 * mode 0, pack_rows_ffn_qkv / pack_rows_ffn for mode 1: proj, 8 chunks of [fc1 rows of 256 hidden units, fc2 columns of the same units],
 * then the next block's qkv; fragment format as omp_dec_rows_ffn).  bf16 matrix-core operands (LayerNorm outputs and hidden activations
 * are rounded to bf16 exactly where the launch-per-Linear path rounds), fp32 accumulation, the bf16 engine's GELU. */
typedef struct {
  int64_t M;
  float eps;
  int32_t mode;
  float* x;
  const void* att;
  void* qkv;
  const void* wstream;
  int64_t wave_stride;
  const float *proj_b, *n2_g, *n2_b, *fc1_b, *fc2_b;   /* mode 1 */
  const float *n1_g, *n1_b, *qkv_b;                    /* the LayerNorm + qkv Linear behind the chain (mode 0: the chain itself) */
  int32_t x3;                                          /* 1 = the parity engine's chain: att split pairs bf16 [M, 1024], qkv fp32 [M, 1536], split weight stream */
} omp_swin_rows_args;
int omp_swin_rows_block(const omp_swin_rows_args* a, omp_stream_t s);

/* ---- Swin patch embedding: zero-pad to x4, 4x4/4 conv (as K=48 dot products), LayerNorm -----
 * Replaces PatchEmbed.forward, swin_transformer.py:427-443.  img is NCHW fp32 (as the reference
 * feeds it); w is the conv weight [E,3,4,4] fp32; out is [B, ceil(H/4)*ceil(W/4), E]. */
int omp_patch_embed_ln(const float* img, const float* w, const float* b, const float* gamma,
                       const float* beta, void* out, int out_dtype, int B, int H, int W, int E,
                       float eps, omp_stream_t s);

/* ---- Fused (shifted-)window attention core -------------------------------------------------------
 * Replaces everything between the qkv and proj Linears of one SwinTransformerBlock:
 * F.pad to x7 (after norm1 => padded tokens carry bias-only q/k/v), torch.roll, window_partition,
 * q*scale, q@k^T + relative_position_bias (+ SW-MSA mask, -100), softmax, @v, window_reverse,
 * roll back, crop.  swin_transformer.py:209-244 + :129-147 + mask construction :369-387.
 * qkv: [B*H*W, 3C] (q|k|v, heads contiguous, head_dim 32); qkv_bias fp32 [3C];
 * rel_bias_table fp32 [(2*7-1)^2, nH]; out: [B*H*W, C].  shift = 0 or 3. */
int omp_swin_window_attn(const void* qkv, const float* qkv_bias, const float* rel_bias_table,
                         void* out, int dtype, int B, int H, int W, int C, int nH, int window,
                         int shift, omp_stream_t s);
/* The same with the relative-position bias EXPANDED once per checkpoint (swin_transformer.py:133-135 re-gathers
 * table[index] on every call): bias_expanded fp32 [nH][64][64] from omp_swin_expand_bias (bias / scale per (query, key),
 * -inf on the padding key slots); rel_bias_table may then be NULL.  out_dtype = dtype, or OMP_BF16X2 with dtype OMP_F32
 * (out is then [B*H*W, 2C] split pairs for the bf16x3 proj GEMM). */
int omp_swin_window_attn2(const void* qkv, const float* qkv_bias, const float* rel_bias_table, const float* bias_expanded,
                          void* out, int dtype, int out_dtype, int B, int H, int W, int C, int nH, int window, int shift,
                          omp_stream_t s);
int omp_swin_expand_bias(const float* rel_bias_table, int nH, float* out, omp_stream_t s);

/* ---- Attention half of a Swin block in one launch (bf16 engine, C = 128 with 4 heads: Swin-B stage 0) ------------
 * Replaces `shortcut = x; x = norm1(x); pad; roll; window_partition; attn(qkv -> softmax -> proj); window_reverse;
 * roll back; crop; x = shortcut + drop_path(x)`, swin_transformer.py:196-247 (SwinTransformerBlock.forward up to the
 * first residual) with WindowAttention.forward (:119-151) inlined: q / k / v, the attention weights and the
 * attention output never reach HBM.  x, out: fp32 residual stream [B*H*W, C] (out may be x: a window reads and writes
 * its own tokens only); ln_gamma / ln_beta: norm1; qkv_w bf16 [3C, C], qkv_b fp32 [3C]; bias_expanded from
 * omp_swin_expand_bias; proj_w bf16 [C, C], proj_b fp32 [C].  The products take bf16 operands exactly where the
 * unfused chain of the bf16 engine rounds (LayerNorm output, q / k / v, P, attention output).
 * OMP_ERR_INVALID for any other C / nH / window. */
int omp_swin_attn_block(const void* x, void* out, const float* ln_gamma, const float* ln_beta, float eps, const void* qkv_w,
                        const float* qkv_b, const float* bias_expanded, const void* proj_w, const float* proj_b, int B, int H,
                        int W, int C, int nH, int window, int shift, omp_stream_t s);
/* The same block for C = 256 with 8 heads (Swin-B stage 1), whose weights fit neither LDS nor registers: wpack is the
 * fragment-major image of qkv.weight and proj.weight written once per checkpoint by model/packing.py::pack_attn_block
 * (bf16 [4 C C]); every wave streams its head's operand fragments from it. */
int omp_swin_attn_block_packed(const void* x, void* out, const float* ln_gamma, const float* ln_beta, float eps, const void* wpack,
                               const float* qkv_b, const float* bias_expanded, const float* proj_b, int B, int H, int W, int C,
                               int nH, int window, int shift, omp_stream_t s);

/* ---- PatchMerging gather + LayerNorm(4C) ------------------------------------------------------------
 * Replaces swin_transformer.py:281-293 (pad to even, 2x2 gather in order (0,0),(1,0),(0,1),(1,1),
 * LN).  x: [B,H,W,C] -> y: [B, ceil(H/2)*ceil(W/2), 4C]; the 4C->2C reduction is a GEMM. */
int omp_patch_merge_gather_ln(const void* x, const float* gamma, const float* beta, void* y,
                              int dtype, int B, int H, int W, int C, float eps, omp_stream_t s);
/* the same with distinct input / output types: fp32 residual stream in, bf16 or split-bf16 (OMP_BF16X2) rows out */
int omp_patch_merge_gather_ln2(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype,
                               int B, int H, int W, int C, float eps, omp_stream_t s);

/* ---- fp32 rows -> split-bf16 pair rows (OMP_BF16X2) ---------------------------------------------------------------
 * y[r, c] = hi = bf16(x[r, c]); y[r, C + c] = lo = bf16(x[r, c] - hi)            (triple = 0: [hi | lo], ldy >= 2C)
 * triple = 1 writes [hi | hi | lo] (ldy >= 3C): the W-side image of an activation (K / V^T projection with swapped
 * operands).  Producers that can write split rows themselves do (omp_layernorm, omp_gemm_bias_act, omp_swin_window_attn2);
 * this is the conversion for the others (FPN output, decoder memory).  No reference counterpart: storage format. */
int omp_split_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int C, int triple, omp_stream_t s);

/* ---- FPN top-down + resample + concat, evaluated only where input_proj samples it -------------
 * Replaces fpn.py:25-44 (nearest top-down adds, bilinear resample of p2/p4/p5 to c3's grid,
 * concat) fused with the stride-`stride` sampling of omniparser.py:15,31.  l2..l5 are the four
 * lateral 1x1-conv outputs (token-major, 256 channels); out: [B, ceil(h3/stride)*ceil(w3/stride),
 * 1024] ordered (p2,p3,p4,p5). */
int omp_fpn_fuse(const void* l2, const void* l3, const void* l4, const void* l5, void* out,
                 int dtype, int B, int h2, int w2, int h3, int w3, int h4, int w4, int h5, int w5,
                 int stride, omp_stream_t s);

/* omp_fpn_fuse at stride 2 on the regular geometry h2 == 2 h3 == 4 h4 (and the widths alike; refused otherwise), reading only the
 * lateral pixels that grid needs: l3s is the [B, h4, w4] map of l3's pixels (2 ty, 2 tx), l2s the [B, 2 h4, 2 w4] map of l2's rows and
 * columns {4 t, 4 t + 1} (omp_layernorm_sampled with step / group = 2 / 1 and 4 / 2, then the lateral products); l4, l5 are whole.
 * out [B, h4 * w4, 1024] equals omp_fpn_fuse's bit for bit; the p3 value under the four p2 taps of an output is summed once. */
int omp_fpn_fuse_sampled(const void* l2s, const void* l3s, const void* l4, const void* l5, void* out, int dtype, int B, int h2,
                         int w2, int h3, int w3, int h4, int w4, int h5, int w5, omp_stream_t s);

/* ---- Padding mask at a feature level: nearest-neighbour resize, exactly F.interpolate(mask[None].float(), size=(h, w))
 * .to(torch.bool)[0] of swin_transformer.py:621 (source index = min(floor(dst * (float)H / h), H - 1)).
 * in: uint8 [B,H,W] (1 = padding), out: uint8 [B,h,w]. */
int omp_mask_nearest(const uint8_t* in, uint8_t* out, int B, int H, int W, int h, int w, omp_stream_t s);

/* ---- Sine position embedding ---------------------------------------------------------------------
 * Replaces PositionEmbeddingSine.forward (normalize=True), backbone/position_embedding.py:24-44.
 * mask: [B,h,w] uint8 (1 = padding); pos: [B, h*w, 2*npf] token-major, (y feats | x feats). */
int omp_sine_posembed(const uint8_t* mask, void* pos, int dtype, int B, int h, int w, int npf,
                      float temperature, omp_stream_t s);

/* ---- Decoder step pieces (KV-cached restatement of transformer.py:74-100,430-454) -----------------
 * All rows of a phase sit at the same sequence position *d_pos (device int32). */

/* x = LN(word_emb[seq[r, *d_pos]] + pos_tab[*d_pos]); writes fp32 x and/or y (dtype).
 * Replaces DecoderEmbeddings.forward, transformer.py:302-328. */
int omp_dec_embed_ln(const int32_t* seq, int seq_ld, const int32_t* d_pos, const float* word_emb,
                     const float* pos_tab, const float* gamma, const float* beta, float* x, void* y,
                     int y_dtype, int R, int d, float eps, omp_stream_t s);

/* Append this step's k,v (from qkv [R,3d]) to the caches [R,Lmax,d] at *d_pos and attend the new
 * query over positions 0..*d_pos (causal self-attention with KV cache; head_dim = d/nH = 64).
 * Replaces self_attn of transformer.py:412-414/:438-440 + generate_square_subsequent_mask.
 * OMP_ERR_INVALID, nothing written: a null pointer, R <= 0, Lmax <= 0, d != 64 nH, a dtype other than OMP_F32 / OMP_BF16.  *d_pos < Lmax
 * is the caller's duty (the position lives in device memory). */
int omp_dec_self_attn_step(const void* qkv, void* kcache, void* vcache, void* out,
                           const int32_t* d_pos, int dtype, int R, int nH, int d, int Lmax,
                           omp_stream_t s);

/* Cross attention of R query rows over per-image memory K / V^T in the head-blocked slabs written by
 * omp_gemm_bias_act(OMP_STORE_KBLK / OMP_STORE_VBLK):  K [image][head][Mpad][64],
 * V^T [image][head][Mpad/KB][64][KB] (KB = 32 bf16 / 16 f32), img_stride = nH*Mpad*64 elements.
 * Rows are grouped by image: groups[g] = {row0, nrows <= 16*q_tiles, image}; a workgroup streams its
 * key range of one (image, head) once for all rows of the group.  Keys are cut in n_split workgroup
 * splits (power of two <= 16) x 4 waves; n_split > 1 goes through `partial`
 * (fp32 [R][nH][n_split][68]) and a merge kernel.  The memory is never replicated per query row.
 * dtype OMP_BF16X2 (round 4, the parity engine): K / Vt are SPLIT-PLANE slabs -- every 32-key block is [hi plane | lo plane] of
 * bf16 (K [image][head][Mpad/32][2][32][64], V^T [image][head][Mpad/32][2][64][32], img_stride = nH*Mpad*128 bf16 elements; the
 * bytes of the fp32 slabs, written by omp_gemm_bias_act with out_dtype OMP_BF16X2 and a blocked store mode), q and out are fp32
 * rows; scores and values run as three bf16 matrix-core products each, i.e. fp32-grade results at the HBM rate.
 * key_mask: NULL or uint8 [B][M], nonzero = padded key (masked).  key_len (ABI 22, ragged batches): NULL, or device int32 [B] with
 * 1 <= key_len[b] <= M: image b's keys are slab positions 0 .. key_len[b]-1 (same slab layout and img_stride); no 32-/16-key block at
 * or beyond ceil(key_len[b] / KB) is loaded, and each image's keys are cut like M keys would be, with key_len[b] in place of M
 * (key_len[b] == M: the same ranges and bits as key_len = NULL).  key_mask, if also given, applies inside key_len.  Slab rows
 * beyond key_len[b] are never read as keys but must not be NaN where a loaded block covers them (dead keys enter P.V with P = 0).
 * Replaces multihead_attn of transformer.py:416-420/:442-446 with memory.repeat (transformer.py:88-96). */
int omp_dec_cross_attn_step(const void* q, int64_t ldq, const void* K, const void* Vt, int64_t img_stride,
                            int Mpad, const uint8_t* key_mask, const int32_t* key_len, const int32_t* groups,
                            int n_groups, int q_tiles, int R, float* partial, void* out, int64_t ldo, int dtype,
                            int M, int nH, int n_split, omp_stream_t s);

/* Greedy sampling of one step from logits [R, ld] fp32: softmax over the support, candidate
 * filtering, argmax, probability; appends the token at seq[r, *d_pos + 1], the probability at
 * probs[r, *d_pos + 1], maintains finished/lengths for the point decoder, then (if advance)
 * increments *d_pos.  Replaces transformer.py:106-129 (pt), :258-263 (poly), :272-282 (rec) and
 * the KIE variants :154-183.  `step0` = sequence position of the first generated token.
 * A wave per row; beyond 1024 rows (OMP355_SAMPLE_BLOCK_MAX_ROWS) with 16-byte aligned rows (ld % 4 == 0) and vocab <= 2048 the row is held in
 * registers (one pass over the logits).  Probabilities may differ in the last bit between the kernels (summation order); tokens do not. */
typedef struct {
  int32_t kind;        /* OMP_DEC_* */
  int32_t num_bins, pt_eos, poly_eos, rec_eos, vocab;
  int32_t vie_categories, infer_vie; /* infer_vie: period-3 pt pattern; poly/rec slice class logits */
  int32_t suppress_eos;              /* forced-length benchmarking: EOS is never selectable */
  int32_t step0;
} omp_sample_cfg;
int omp_head_softmax_mask_argmax(const float* logits, int ld, int R, const omp_sample_cfg* cfg,
                                 int32_t* seq, float* probs, int seq_ld, int32_t* finished,
                                 int32_t* lengths, int32_t* d_pos, int advance, omp_stream_t s);

/* ---- Results of an engine call -> padded tensors (payload of the per-call all-gather) --------------------------
 * Replaces the per-image result assembly of engine/val.py:39-60 for a batch: instance n of image b is row row0[b] + n of
 * points [R,2], poly [R, poly_ld >= 32], rec [R, rec_ld >= rec_len], rec_probs [R, prob_ld] (device int32 / fp32, the
 * decoders' own buffers); ids [B, N, 2 + 32 + rec_len] int32 = point | polygon | recognition tokens, probs [B, N, rec_len];
 * instances beyond counts[b] (or N) are zero. */
int omp_pack_spotting(const int32_t* points, const int32_t* poly, int poly_ld, const int32_t* rec, int rec_ld,
                      const float* rec_probs, int prob_ld, const int32_t* row0, const int32_t* counts, int B, int N,
                      int rec_len, int32_t* ids, float* probs, omp_stream_t s);

/* ---- One decoder, many steps (the launch-bound inner loop runs from C++, optionally as a
 *      hipGraph replay).  Replaces Transformer.decode driven by decode_pt_seq / the poly and rec
 *      loops, transformer.py:74-141,252-284. */
typedef struct {
  const void* sa_in_w;         /* [3d,d] */
  const float* sa_bias_tab;    /* [Pmax,3d]: in_proj_bias + pos_tab @ [Wq;Wk;0]^T */
  const void* sa_out_w;
  const float* sa_out_b;
  const void* ca_q_w;          /* [d,d] */
  const float* ca_qbias_tab;   /* [Pmax,d] */
  const void* ca_out_w;
  const float* ca_out_b;
  const void* ff1_w;
  const float* ff1_b;
  const void* ff2_w;
  const float* ff2_b;
  const float *n1_g, *n1_b, *n2_g, *n2_b, *n3_g, *n3_b;
  void* kcache;                /* [R,Lmax,d] */
  void* vcache;
  const void* crossK;          /* this layer's K slab   [B][nH][Mpad][64] */
  const void* crossVt;         /* this layer's V^T slab [B][nH][Mpad/KB][64][KB] */
  /* row-owner chains (omp_decoder_plan.rows_fused, see omp_dec_rows_mid / omp_dec_rows_ffn): packed weight streams of this layer */
  const void* rows_mid;        /* sa_out_w, ca_q_w.  Bound on EVERY layer of a bf16 pre-norm plan WITHOUT rows_fused (d_model 512, 8 heads, more than 63 rows), it
                                  makes the launch-per-Linear step run out-projection + residual, norm2 and the cross-attention query as ONE omp_dec_rows_mid
                                  launch (16-row workgroups) instead of three; NULL: three launches */
  const void* rows_ffn;        /* ca_out_w, ff1_w / ff2_w in 16 chunks, then the NEXT layer's sa_in_w -- the last layer: h0_w, h1_w, h2_w */
  /* bytes between the streams of consecutive waves, AS RETURNED BY THE PACKER that wrote the stream (model/packing.py::pack_rows_*: fragments per
   * wave x 1 KB).  The kernels know how many fragments each chain consumes; omp_decoder_run refuses a plan whose strides differ (a packer or
   * layout change must fail loudly, not mis-stream weights). */
  int64_t rows_mid_stride, rows_ffn_stride;
} omp_dec_layer;

typedef struct {
  int32_t dtype, n_layers, d_model, n_heads, d_ff, vocab, pre_norm;
  int32_t R, Lmax, M, Mpad, n_tiles, q_tiles, n_split, n_prompt; /* n_tiles = row groups, see omp_dec_cross_attn_step */
  /* gemm_x3 = 1 (dtype OMP_F32, pre_norm, R > 64: the many-row phases of the bf16x3 engine): every matrix pointer below
   * (sa_in_w ... ff2_w, h0_w ... h2_w) is the [out, 3 * in] bf16 image [w_hi | w_hi | w_lo] of the fp32 weight and the step's
   * products run as split-bf16 products (omp_gemm_args.a_wrap); activations, caches, slabs and every other kernel stay fp32. */
  int32_t gemm_x3;
  /* kv_split = 1 (dtype OMP_F32): crossK / crossVt are split-plane slabs (OMP_BF16X2 with OMP_STORE_KBLK / OMP_STORE_VBLK, 32-key
   * blocks of [hi plane | lo plane]); q and the attention output stay fp32 (with gemm_x3 the kernels write the out-projection's
   * pair rows themselves).  kv_img_stride then counts bf16 elements: nH * Mpad * 128. */
  int32_t kv_split;
  /* rows_fused = 1 (dtype OMP_BF16, or OMP_F32 with gemm_x3: the parity engine's chains over split operands; pre_norm, d_model 512, d_ff 2048,
   * 8 heads; the host sets it for phases of thousands of rows): the
   * Linear layers of a step run as row-owner chains -- omp_dec_rows_ffn(embedding | q k v), then per layer self-attention,
   * omp_dec_rows_mid, cross-attention, omp_dec_rows_ffn -- 18 launches per step instead of 50; layers[l].rows_mid / rows_ffn and
   * rows_embed (layer 0's sa_in_w) are the packed streams (model/packing.py::pack_rows_*). */
  int32_t rows_fused;
  /* XCD placement of the chains' workgroups (round 6; speed only, never correctness).  Bit x set = XCD x may run them; 0 = all eight.  The
   * dispatcher is observed to place block b on XCD b % 8: a chain launch of at most 32 x popcount(mask) workgroups is launched with the blocks of
   * the other XCDs retiring at once, so that its weight stream fills popcount(mask) private L2s instead of eight (the polygon decoder's chains
   * 0x0F, the recognition decoder's 0xF0: each weight set lives in four L2s).  Larger launches ignore it. */
  int32_t rows_xcd_mask;
  float eps;
  const void* rows_embed;
  int64_t rows_embed_stride;   /* as layers[].rows_*_stride */
  omp_dec_layer layers[OMP_MAX_DEC_LAYERS];
  const float *word_emb, *pos_tab, *emb_g, *emb_b, *fn_g, *fn_b;
  const void *h0_w, *h1_w, *h2_w;
  const float *h0_b, *h1_b, *h2_b;
  int64_t kv_img_stride;
  const uint8_t* key_mask;     /* NULL or uint8 [B][M], nonzero = padded key; see omp_dec_cross_attn_step */
  const int32_t* key_len;      /* NULL or device int32 [B], 1 <= key_len[b] <= M: ragged batches, see omp_dec_cross_attn_step (ABI 22).
                                  Read by every step, so a graph_slot replay sees the buffer's contents at replay time */
  const int32_t* tiles;
  /* state */
  int32_t* seq;
  int32_t seq_ld;
  int32_t* d_pos;  /* int32[2]: {current position, ticket word of the sampling kernel (zero-initialised by the caller)} */
  float* probs;
  int32_t* finished;
  int32_t* lengths;
  /* scratch */
  float* x;      /* [R,d] fp32 residual stream */
  float* x2;     /* [R,d] fp32 (post-norm temp) */
  void* y;       /* [R,d] */
  void* qkv;     /* [R,3d] */
  void* att;     /* [R,d] */
  void* q;       /* [R,d] */
  void* ffh;     /* [R,d_ff] */
  void* hh0;     /* [R,d] */
  void* hh1;     /* [R,d] */
  float* partial;
  float* logits; /* [R,vocab] */
  omp_sample_cfg sample;
  /* Batched prompt prefill (the members behind `sample`).  The prompt tokens are known before the first launch, and all that positions 0 .. n_prompt - 2
   * leave behind is the self-attention K / V cache rows of those positions.  With prefill != 0 an ELIGIBLE plan runs them as ONE pass
   * over L = n_prompt - 1 positions when omp_decoder_run starts at first_pos == 0 with n_steps >= L: R * L prefill rows, row r * L + j
   * = plan row r at position j; every layer but the last in full, the last one up to its self-attention's cache append; no head, no
   * sampling; *d_pos = L afterwards, the ticket word untouched.  Cross-attention streams an image's K / V^T slabs once per group of
   * prefill_tiles -- ceil(R_img * L / (16 * q_tiles)) passes per image instead of L * ceil(R_img / (16 * q_tiles)) -- with the
   * plan's own q_tiles and n_split, i.e. the step's kernel, key ranges and merge.  Every row runs the operations of the stepwise
   * prefill in the same order: caches, ids and probabilities are the same bits.
   * Eligible: dtype OMP_BF16, pre_norm, no rows_fused / gemm_x3 / kv_split, n_prompt >= 3, 64 <= R < 1024 (the launch-per-Linear step
   * with one self-attention wave per (row, head)), R * L <= 4096, no forced GEMM kernel, not the fused few-row step.  Every other plan
   * runs the stepwise prefill whatever `prefill` says.  An eligible plan with prefill set and a table or scratch too small is refused. */
  int32_t prefill;               /* switch: 0 = stepwise prefill */
  int32_t n_prefill_tiles;       /* groups in prefill_tiles */
  const int32_t* prefill_tiles;  /* {row0, nrows <= 16 * q_tiles, image} over the R * L prefill rows: an image's R_img * L rows are contiguous */
  int64_t pf_rows;               /* rows each pf_* buffer holds, >= R * L */
  float* pf_x;                   /* [pf_rows, d] fp32 */
  void* pf_qkv;                  /* [pf_rows, 3d] */
  void* pf_att;                  /* [pf_rows, d] (also holds the LayerNorm outputs between its uses) */
  void* pf_q;                    /* [pf_rows, d] */
  void* pf_ffh;                  /* [pf_rows, d_ff] */
  float* pf_partial;             /* fp32 [pf_rows][n_heads][n_split][68] (n_split > 1) */
} omp_decoder_plan;

/* Runs steps for input positions first_pos .. first_pos+n_steps-1 (host-side counter must match
 * *d_pos).  Positions < n_prompt-1 are prompt prefill (no head / sampling): one eager step each, or -- omp_decoder_plan.prefill --
 * one batched pass for all of them.  graph_slot >= 0
 * caches a hipGraph of the sampling step under that slot (call omp_decoder_graph_reset when the
 * plan's pointers or shapes change); graph_slot < 0 launches eagerly. */
int omp_decoder_run(const omp_decoder_plan* plan, int first_pos, int n_steps, int graph_slot,
                    omp_stream_t s);
int omp_decoder_graph_reset(int graph_slot);
/* The capture gate (round 6, ABI 21; no reference counterpart: engine/val.py:19-35 runs one image at a time on one thread).  omp_decoder_run
 * captures a graph on the caller's stream the first time a graph_slot is used.  While a stream captures, HIP fails -- and invalidates the
 * capture on -- hipEventSynchronize / hipEventQuery / hipStreamWaitEvent of every event LAST RECORDED IN THAT STREAM, events of earlier,
 * uncaptured work included (hipErrorCapturedEvent / hipErrorStreamCaptureIsolation).  A host thread that waits on an event recorded in a
 * stream which ANOTHER thread drives through omp_decoder_run must bracket the event call with enter / leave: a capture holds the same
 * process-wide mutex from begin to instantiate.  Keep the bracket non-blocking (query, stream-wait; poll instead of hipEventSynchronize) and
 * never call omp_decoder_run inside it.  Not needed for events of the calling thread's own streams.  Always OMP_OK. */
int omp_capture_gate_enter(void);
int omp_capture_gate_leave(void);
/* Two decoders' many-row phases as ONE interleaved schedule (round 6; the polygon and recognition loops of Transformer.forward,
 * transformer.py:252-284, which depend on the points only).  Both plans must be rows_fused plans with the same number of layers.
 * Positions first_pos .. first_pos + max(n_steps_a, n_steps_b) - 1: while both decoders have steps left, every cross-attention kernel of
 * both goes to the ONE stream sx in the order a[0], b[0], a[1], b[1] ..., chained by events to the decoders' own streams sa / sb, which
 * carry everything else (self-attention, the row-owner chains, sampling): one decoder's chains -- matrix-core work on half the compute
 * units -- run beside the OTHER decoder's HBM-bound cross-attention instead of beside its own kind.  sa and sb should be created with a
 * HIGHER priority than sx (a chain workgroup needs a whole CU's LDS: the queue priority decides who is placed when a launch drains).  The
 * longer decoder finishes alone on its stream.  Eager launches; three distinct non-default streams; the caller joins sa and sb afterwards.
 * Results are the same bits as two omp_decoder_run calls (the same kernels on the same operands: only WHEN they run changes). */
int omp_decoder_run_pair(const omp_decoder_plan* plan_a, const omp_decoder_plan* plan_b, int first_pos, int n_steps_a, int n_steps_b,
                         omp_stream_t sa, omp_stream_t sb, omp_stream_t sx);

/* ---- Many-row decoder phases: the Linear chain between two attention kernels as ONE launch (round 5, csrc/dec_rows.hip) -----------
 * Replaces, for phases of thousands of rows (polygon / recognition decoders of a large engine call), the per-Linear launches of
 * TransformerDecoderLayer.forward_pre, transformer.py:430-454, at d_model 512 / d_ff 2048 / bf16 operands:
 *   omp_dec_rows_mid:  x += att Wo^T + bo  (self-attention out-projection + residual, :438-440);
 *                      q  = bf16(LayerNorm2(x) Wq^T + qbias_tab[*d_pos])  (:441-446, query side of multihead_attn)
 *   omp_dec_rows_ffn:  prologue 0: x1 = x + att Wo^T + bo (cross-attention out-projection + residual, :442-447);
 *                                  x  = x1 + relu(LayerNorm3(x1) W1^T + b1) W2^T + b2  (:448-453)
 *                      prologue 1: x  = LayerNorm(word_emb[seq[r, *d_pos]] + pos_tab[*d_pos])  (DecoderEmbeddings, :302-328: layer 0)
 *                      tail 0:     qkv = bf16(LayerNorm_t(x) Win^T + bias_tab[*d_pos])  (the NEXT layer's norm1 + in_proj, :437-440)
 *                      tail 1:     logits = h2(relu(h1(relu(h0(LayerNorm_t(x))))))  (decoder norm :374 + prediction head, block/mlp.py:11-13)
 * A workgroup owns omp_dec_rows_tile() consecutive rows (operand tile in LDS, residual / accumulators in registers) and streams the
 * chain's weights; every wave w (8 per workgroup) walks its own linear stream of 1 KB matrix-core fragments starting at
 * wstream + w * wave_stride, written once per checkpoint by model/packing.py::pack_rows_* in consumption order:
 *   a product of N = 512 (128) output features over K: for each k-step of 32, for each of the wave's 4 (1) feature tiles of 16 --
 *   features 64 w + 16 t .. (16 w ..) of the pass --: fragment[lane][8] = W[f0 + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8];
 *   the FFN interleaves, per chunk of 256 hidden units, linear1's pass (N = 256: features 32 w + 16 t, t = 0..1, K = 512) with linear2's
 *   (N = 512, K = 256);
 *   the vocabulary projection is padded with zero rows to a multiple of 128 features (512-feature passes, then 128-feature passes).
 * wave_stride must equal (fragments of the chain per wave) x 1 KB -- what the packer returns; the entry points refuse anything else.
 * The buffer carries PF x 1 KB of slack behind the last wave's stream, PF = fragments the kernels keep in flight (the ring runs ahead of the
 * stream's end): 8 KB for the bf16 chains, 16 KB for the x3 chains (pairs of hi / lo fragments); model/packing.py allocates 16 KB for both.
 * att: bf16 [R, 512]; x: fp32 [R, 512] in place; q: bf16 [R, 512]; qkv: bf16 [R, 1536]; logits: fp32 [R, vocab], vocab % 4 == 0. */
typedef struct {
  int32_t R;
  float eps;
  const int32_t* d_pos;
  float* x;
  const void* att;
  const void* wstream;
  int64_t wave_stride;
  const float* out_b;
  const float *ln_g, *ln_b;        /* mid: norm2; ffn prologue 0: norm3 */
  const float* qbias_tab;          /* mid: [Pmax, 512] */
  void* q;                         /* mid */
  int32_t prologue, tail;          /* ffn */
  const float *ff1_b, *ff2_b;
  const int32_t* seq;
  int32_t seq_ld;
  const float *word_emb, *pos_tab, *emb_g, *emb_b;
  const float *lnt_g, *lnt_b;      /* the LayerNorm in front of the tail */
  const float* bias_tab;           /* tail 0: [Pmax, 1536] */
  void* qkv;
  const float *h0_b, *h1_b, *h2_b; /* tail 1 */
  float* logits;
  int32_t vocab;
  /* x3 = 1: the PARITY engine's chains (csrc/dec_rows.hip, SplitRows): every product as three bf16 matrix-core products of split operands.  att is then
   * split pairs bf16 [R, 1024] = [hi | lo] (omp_split_bf16 / the split-plane cross-attention), q / qkv are fp32 [R, 512] / [R, 1536], and
   * wstream carries per (k-step, feature tile) the fragment of w_hi then of w_lo (twice the fragments; model/packing.py, x3=True); a
   * workgroup owns 48 rows. */
  int32_t x3;
  int32_t xcd_mask;                /* XCDs whose CUs may run the launch's workgroups (omp_decoder_plan.rows_xcd_mask); 0 = all */
  int32_t pos_mod;                 /* omp_dec_rows_mid, bf16 chains: > 0 = row r sits at position r % pos_mod and d_pos is not read (the batched prompt
                                      prefill of omp_decoder_run); 0 = every row at *d_pos */
} omp_dec_rows_args;
int omp_dec_rows_mid(const omp_dec_rows_args* a, omp_stream_t s);
int omp_dec_rows_ffn(const omp_dec_rows_args* a, omp_stream_t s);
int omp_dec_rows_tile(void);   /* the LARGEST tile: 80 rows per workgroup (the Swin chains always; decoder launches take 16 x {1..5} rows: the smallest
                                  tile that keeps the launch on half the device's compute units, csrc/dec_rows.hip rows_rtt) */

/* Cross-attention memory projection as a row-owner stream kernel (csrc/kv_rows.hip, round 5) -- replaces, for bf16 engines with d_model 512,
 * 8 heads and M % 64 == 0, the two omp_gemm_bias_act launches with OMP_STORE_KBLK / OMP_STORE_VBLK that computed what nn.MultiheadAttention
 * recomputes per step and instance (model/transformer.py:88-96, 442-446).  rows: [B * M, 512] bf16 memory rows (memory + pos for K, memory
 * for V^T); wstream: the [n_slabs * 512, 512] projection weights of all (decoder, layer) pairs as per-wave fragment streams
 * (model/packing.py::pack_kv_rows_k -- dims permuted per head so that a lane stores 16 consecutive dims -- / pack_kv_rows_v), wave_stride
 * bytes apart; bias [n_slabs * 512] fp32; out: the slab base, K [slab][B][8][Mpad][64] (vt = 0) or V^T [slab][B][8][Mpad / 32][64][32] in the
 * key-slot order of OMP_STORE_VBLK (vt = 1).  The padded tail (keys >= M) is not written.  Bit-identical to the tiled GEMM path. */
int omp_kv_project_rows(const void* rows, const void* wstream, int64_t wave_stride, const float* bias, void* out, int B, int M, int Mpad,
                        int n_slabs, int vt, omp_stream_t s);

/* ---- MGP-STR recogniser (reference: OCR/MGP-STR; BASELINE config 5) ------------------------------------
 * The ViT-B encoder reuses omp_layernorm / omp_gemm_bias_act / omp_dec_cross_attn_step (a ViT layer's k and v
 * projections write the blocked slabs, an image's 257 tokens are row groups of that image); these three entry
 * points cover what is specific to MGP-STR. */

/* bf16 self-attention of a ViT layer, all heads of all images in one launch: out[b*T + i, h*64 + :] =
 * softmax_j(q_i . k_j / 8) v_j.  Replaces timm Attention.forward (the blocks modules/mgp_str.py:71-74 runs).
 * q [B*T, ldq] (head h at columns h*64), K / Vt = one layer's blocked slabs [B][nH][Mpad][64] and
 * [B][nH][Mpad/32][64][32] as written by omp_gemm_bias_act with OMP_STORE_KBLK / OMP_STORE_VBLK (kv_key_block 32),
 * padded keys zero.  Built for dtype OMP_BF16 and Mpad == 288 (T <= 288, MGP-STR: 257); other shapes return
 * OMP_ERR_UNSUPPORTED and are served by omp_dec_cross_attn_step on the same slabs. */
int omp_vit_attn(const void* q, int64_t ldq, const void* K, const void* Vt, int Mpad, void* out, int64_t ldo,
                 int dtype, int B, int T, int nH, omp_stream_t s);
/* The same attention on ONE token-major projection qkv [B T, 3 nH 64] = [q | k | v] (timm's fused qkv Linear, modules/mgp_str.py:72-73; round 6): the key
 * rows reach LDS by strided DMA and the kernel builds the blocked V^T image itself, so the projection is one plain product of N = 3 nH 64 instead of a
 * plain one and two with blocked-slab epilogues (the V^T slab store costs 2.7x a plain product at 257 tokens per image).  bf16, T <= 288. */
int omp_vit_attn_qkv(const void* qkv, int64_t ld, void* out, int64_t ldo, int dtype, int B, int T, int nH, omp_stream_t s);

/* Patch embedding + cls token + position embedding.  Replaces timm PatchEmbed (Conv2d(3,E,4,4) -> flatten ->
 * transpose) and modules/mgp_str.py:66-70.  img NCHW fp32 [B,3,H,W] (H, W multiples of 4); w [E,3,4,4], bias [E],
 * cls [E], pos [(H/4)*(W/4)+1, E] fp32; out [B, (H/4)*(W/4)+1, E] token-major, token 0 = cls. */
int omp_vit_patch_embed(const float* img, const float* w, const float* bias, const float* cls, const float* pos,
                        void* out, int out_dtype, int B, int H, int W, int E, omp_stream_t s);

/* A^3 module core, modules/token_learner.py:27-31: maps[b,s,:] = softmax over the T tokens of sel[b,:,s];
 * pooled[b,s,:] = sum_i maps[b,s,i] * feat[b,i,:].  sel fp32 [B*T, ld_sel] (S <= 28 columns), feat [B*T, C]
 * (dtype), pooled fp32 [B*S, C], attn fp32 [B,S,T] or NULL. */
int omp_a3_pool(const float* sel, int ld_sel, const void* feat, int dtype, float* pooled, float* attn, int B, int T,
                int S, int C, omp_stream_t s);

/* Greedy decoding WITHOUT materialising the logits (round 6; MGP-STR's BPE / WordPiece heads: 13 824 rows x 50 257 / 30 522 classes are 2.8 / 1.7 GB
 * of fp32 per forward that the head product writes and the arg-max pass reads back -- test_final.py:145-170 needs only the greedy id and its
 * softmax probability).  omp_gemm_bias_act with store_mode = OMP_STORE_ROWSTAT (out_dtype f32; no residual / activation / second destination /
 * transposed output) runs the product on 128 x 128 tiles and, instead of the logits, stores per (row, column tile) the tile's statistics into
 * C = float [M][2 ceil(N / 128)][4], one record per 64-column half tile: {maximum of logit + bias, sum of exp(logit - maximum), index of the
 * maximum (int32 bits, lowest index on ties), 0}; a half without a valid column holds {-inf, 0, .}.  omp_row_stat_merge folds a row's tiles: ids[r] = arg max, prob[r] = 1 / sum_tiles s_t exp(m_t - max) -- the values
 * omp_row_argmax_prob computes from the full row (same product bits; the probability differs by the rounding of a different summation order). */
int omp_row_stat_merge(const float* stats, int R, int n_records, int32_t* ids, float* prob, omp_stream_t s);   /* n_records = 2 ceil(N / 128) */
/* Greedy id and its softmax probability for every row of logits fp32 [R, ld] (V columns used).  Replaces
 * topk(1) + softmax(...).max(dim=2) of test_final.py:145-170. */
int omp_row_argmax_prob(const float* logits, int64_t ld, int R, int V, int32_t* ids, float* prob, omp_stream_t s);

/* ---- context: ALL mutable state of the library ---------------------------------------------------
 * An omp_ctx holds the table of hipGraphs that omp_decoder_run captures under its graph_slot ids, plus the development
 * state declared in csrc/omp355_debug.h (kernel selectors, trace buffers, measurement brackets).  Every entry point
 * works on the CURRENT context of the calling host thread: the process default context until the thread calls
 * omp_ctx_make_current.  Two engines in one process (or one per pipeline lane) get independent state by creating
 * their own; destroying a context destroys the graphs it captured.  Beyond the context the library keeps only a
 * thread-local error string.  Scratch memory is owned by the caller (every buffer is an argument; omp_decoder_plan
 * lists the decoder's), so there is no omp_workspace_bytes to query. */
typedef struct omp_ctx omp_ctx;
int omp_ctx_create(omp_ctx** out);
int omp_ctx_destroy(omp_ctx* ctx);          /* not the default context */
int omp_ctx_make_current(omp_ctx* ctx);     /* NULL = back to the process default context */
omp_ctx* omp_ctx_current(void);             /* the calling thread's context (never NULL) */

/* ---- test-time image pre-processing (the step before the hot path) -----------------
 * Replaces dataset/transforms.py:249-298 (RandomResize([test_min_size], test_max_size) = Pillow bilinear resize
 * through torchvision F.resize), :312-322 (ToTensor, Normalize) and the padding / mask construction of
 * utils/nested_tensor.py:37-54 for ONE image of a batch.  src: uint8 HWC RGB on the device.  xbounds/xcoef,
 * ybounds/ycoef: Pillow's coefficient tables ([out][2] = first source index, count; [out][ks] 22-bit fixed point;
 * utils/preprocess.py builds them; may be NULL for an axis whose size does not change).  lut: float [3][256] =
 * ((p / 255) - mean_c) / std_c.  dst: this image's [3, dst_h, dst_w] fp32 slice of the batch tensor; mask: its
 * [dst_h, dst_w] uint8 slice (1 = padding) or NULL.  Bit-exact with the reference pipeline. */
int omp_resize_normalize_pad(const uint8_t* src, int64_t src_pitch, int in_h, int in_w, const int32_t* xbounds,
                             const int32_t* xcoef, int ksx, const int32_t* ybounds, const int32_t* ycoef, int ksy,
                             const float* lut, float* dst, uint8_t* mask, int out_h, int out_w, int dst_h,
                             int dst_w, omp_stream_t s);

/* ---- word crops for the recogniser, a chunk per launch ------
 * The reference ships no glue between its spotter and its recogniser; these two stand for what a curved-text reader
 * puts there (BezierAlign and its relatives) followed by MGP-STR's own crop transform (OCR/MGP-STR/dataset.py:462:
 * image.resize((imgW, imgH), Image.BICUBIC) + ToTensor), for ALL crops of a chunk at once.  Descriptor tables live in
 * device memory, one row per crop; utils/word_crops.py packs them. */
typedef struct omp_rectify_desc {
  const uint8_t* src;   /* the crop's source image: uint8 HWC RGB on the device */
  int64_t pitch;        /* bytes per source row */
  int32_t w, h;         /* source size: sample coordinates clamp to it */
  int32_t sh, sw;       /* strip size, each in [1, 4096] */
  int64_t strip_off;    /* byte offset of the packed sh x sw x 3 strip in the scratch buffer */
  int64_t tile0;        /* tiles (64 columns x 4 rows) of all earlier crops: ascending, 0 for the first */
  int64_t pq[32];       /* the 16 (x, y) points in original-image pixels, 16 fractional bits: 8 along the top edge in
                           reading order, then 8 along the bottom edge walking back (utils/misc.py: bezier2polygon) */
} omp_rectify_desc;
typedef struct omp_resize_desc {
  const uint8_t* src;   /* uint8 HWC RGB crop on the device (a strip, or a box of an image) */
  int64_t pitch;        /* bytes per crop row */
  int32_t in_h, in_w;
  int32_t xb, kx, ksx;  /* offsets (in int32 entries) of the x bounds [out_w][2] and coefficients [out_w][ksx] in the packed
                           table; ksx = 0: the width does not change */
  int32_t yb, ky, ksy;  /* the same for y */
} omp_resize_desc;
/* Samples every crop's source image along its polygon into its strip (integer bilinear, 16 fractional bits; the map is
 * written out in utils/word_crops.py: rectify_polygon_cpu, which this equals byte for byte).  One launch of total_tiles
 * workgroups = the sum over crops of ceil(sw / 64) * ceil(sh / 4).  Strips that would not fit scratch_bytes are not
 * written. */
int omp_polygon_rectify(const omp_rectify_desc* desc, int n, int64_t total_tiles, uint8_t* scratch,
                        int64_t scratch_bytes, omp_stream_t s);
/* The batched form of omp_resize_normalize_pad for crops: Pillow's 8-bit resampler with the tables each descriptor
 * points to in ONE packed int32 table, then lut (float [3][256]).  dst: fp32 [n, 3, out_h, out_w].  One launch. */
int omp_resize_crops(const omp_resize_desc* desc, int n, const int32_t* table, int64_t table_len, const float* lut,
                     float* dst, int out_h, int out_w, omp_stream_t s);

/* ---- lexicon correction: the nearest dictionary word of every query -------------
 * Plain Levenshtein distance (insert / delete / substitute cost 1, no transpositions): the distance the reference's
 * recogniser evaluation is built on (OCR/MGP-STR/test_final.py:14, nltk.metrics.distance.edit_distance).  The glue
 * between a reader and a word list ships with neither reference project; utils/lexicon.py holds the specification
 * (edit_distance_cpu, nearest_cpu) and packs the operands:
 *   q_codes  uint8 [n][64]: the queries as alphabet indices; 254 = a character outside the alphabet
 *   q_len    int32 [n]: characters per query, 0..64.  A length outside that range is REFUSED on the device: best[q] = all ones
 *   q_lo, q_hi  int32 [n] each, or both NULL: query q searches the lexicon indices [q_lo[q], q_hi[q]), CLAMPED on the
 *            device to [0, L]; NULL = the whole lexicon
 *   pool     uint8 [pool_bytes]: the lexicon's words back to back as alphabet indices; 255 = a character outside the
 *            alphabet (254 and 255 match nothing, each other included)
 *   offsets  int32 [L + 1]: word i is pool[offsets[i] .. offsets[i + 1]), at most 255 characters; entries are clamped
 *            into the pool on the device, so no table can make the kernel read outside pool[0 .. pool_bytes)
 *   range_hint  the longest range of the call if the caller knows it, else 0: sizes the grid only, never the result
 *   best     uint64 [n], written by this call (a fill launch ahead of the search launch on the same stream; the caller
 *            initialises nothing): (dist << 32) | index of the nearest word of the range, the lowest index among equals;
 *            all ones for an empty range or a refused query.
 * Two launches (fill + search) whatever n and L; no allocation, no synchronisation. */
int omp_lexicon_nearest(const uint8_t* q_codes, const int32_t* q_len, const int32_t* q_lo, const int32_t* q_hi, int n,
                        const uint8_t* pool, int64_t pool_bytes, const int32_t* offsets, int L, int range_hint,
                        uint64_t* best, omp_stream_t s);

/* ---- posterior lexicon decoding: the lexicon word MGP-STR's character head finds most likely ----
 * The character head is non-autoregressive, so P(word) = prod_i p_i(word[i]) * p_len([s]) is the exact probability that
 * the reference's decoding rule (OCR/MGP-STR/test_final.py:172-181) yields the word.  utils/lexicon_post.py holds the
 * specification (costs_cpu, greedy_cpu, score_cpu and the pure-Python score_py).  Floats end at the costs:
 *   logits   float [n][27][38], contiguous: the character head's logits; position 0 is dropped, as recognize does
 *   costs    int32 [n][26][38], written by this call: clip(floor(-log_softmax * 1024 + 0.5), 0, 2^20 - 1), one unit =
 *            1/1024 nat; max, sum of exp and log in fp32, so a cost may differ from costs_cpu (float64) by one unit at a
 *            rounding boundary and by no more
 *   greedy   int32 [n][2], written by this call from the quantised costs: (sum of the per-position least costs through the
 *            first position whose least class is 1 = [s], that position); (26 terms, 26) without one.  Lowest class among equals.
 * One launch of n workgroups; no allocation, no synchronisation.  n <= 0 or a null pointer: OMP_ERR_INVALID, nothing launched. */
int omp_logprob_costs(const float* logits, int n, int32_t* costs, int32_t* greedy, omp_stream_t s);
/* The search.  score(q, w) = sum_{i < len} costs[q][i][class_table[w[i]]] + costs[q][len][1]; integers only, every output
 * equals score_cpu.
 *   costs    int32 [n][26][38] as above (any int32 in [0, 2^20) keeps 26 terms far below 2^31)
 *   q_lo, q_hi  int32 [n] each, or both NULL: query q searches the lexicon indices [q_lo[q], q_hi[q]), CLAMPED on the device
 *            to [0, L]; an inverted range is empty; NULL = the whole lexicon
 *   pool, pool_bytes, offsets, L  the lexicon as omp_lexicon_nearest takes it.  Word i is pool[s, e) with
 *            s = clip(offsets[i], 0, pool_bytes), e = clip(offsets[i + 1], s, pool_bytes): a falling or overlong table never
 *            makes the kernel read outside pool[0 .. pool_bytes).  A word longer than 25 codes is SKIPPED, not truncated
 *   class_table  uint8 [256]: lexicon code -> class 2..37; any other entry (255 by convention) = unscorable: a word that
 *            holds such a code is skipped
 *   range_hint  the longest range of the call if the caller knows it, else 0: sizes the grid only, never the result
 *   best     uint64 [n][2], written by this call (the caller initialises nothing): [q][0] the least key (score << 32) | index
 *            of the range, the lowest index among equals; [q][1] the least key among the OTHER indices (the runner-up; a
 *            duplicate spelling at another index counts); all ones where there is none
 *   work     uint64 [2 * (n + 4096)], caller-owned scratch: the per-slice pairs between the two launches
 * Two launches (search, merge) whatever n and L; the result does not depend on scheduling; no allocation, no synchronisation,
 * no atomics.  A null pointer, q_lo without q_hi, n <= 0, L <= 0, pool_bytes < 0 or range_hint < 0: OMP_ERR_INVALID, nothing
 * launched and nothing written. */
int omp_lexicon_posterior(const int32_t* costs, int n, const int32_t* q_lo, const int32_t* q_hi, const uint8_t* pool,
                          int64_t pool_bytes, const int32_t* offsets, int L, const uint8_t* class_table, int range_hint,
                          uint64_t* best, uint64_t* work, omp_stream_t s);

/* ---- window prompts: the points of a finished point phase, compacted on the device ----
 * The point decoder's prompt holds a spatial window; an engine call may run several windows per image as rows of ONE point
 * phase (the reference's forward takes any such prompt, model/transformer.py:102-141; its training draws them,
 * dataset/collate_fn.py:46-115).  This entry point is the step between that phase and the polygon / recognition phases; it
 * reads the phase's buffers as the sampling kernels left them (omp_decoder_plan.seq / finished / lengths):
 *   seq        int32 [rows][seq_ld]: row r = its prompt (seq[r][0..3] = its window x0, y0, x1, y1), then the sampled tokens
 *   finished, lengths  int32 [rows]: EOS flag and EOS position of every row (omp_head_softmax_mask_argmax)
 *   row_image  int32 [rows]: the image of every row, in [0, n_images); rows outside that range count for no image
 *   n_prompt, sampled  row r's tokens are seq[r][n_prompt .. end), end = lengths[r] if finished[r] else n_prompt + sampled, clamped
 *              into [n_prompt, seq_ld]; an odd tail is dropped (transformer.py:138-139); the tokens are (x, y) pairs
 *   clip       nonzero: keep a pair only if x0 < x <= x1 and y0 < y <= y1 against the row's own window (collate_fn.py:80-81,
 *              verbatim: the lower bounds are strict, so the default window drops bin 0 too).  Needs n_prompt >= 4.
 * Outputs, all int32 and all written by this call (the caller initialises nothing):
 *   points [cap][2], inst_row [cap]: the kept pairs and their rows, in row order and inside a row in the decoder's order (a
 *              stable compaction); entries at or beyond cap are not written (row_start[rows] still holds the full total)
 *   row_count [rows], dropped [rows]: pairs kept / removed by the clip per row
 *   row_start [rows + 1]: exclusive prefix sum of row_count; row_start[rows] = the total
 *   image_count [n_images]: pairs kept per image (through row_image)
 * utils/windows.py: gather_points_cpu is the specification; every output integer equals it.  Three launches (count, scan,
 * copy); no allocation, no synchronisation. */
int omp_window_points(const int32_t* seq, int seq_ld, const int32_t* finished, const int32_t* lengths, const int32_t* row_image,
                      int rows, int n_images, int n_prompt, int sampled, int clip, int32_t* points, int32_t* inst_row, int cap,
                      int32_t* row_count, int32_t* dropped, int32_t* row_start, int32_t* image_count, omp_stream_t s);

/* ---- overlap suppression: which decoded polygons are the same word -------------
 * Neither reference project removes duplicate detections (shapely is in OmniParser's requirements and nothing imports it); windows
 * that overlap, the whole-page window next to a grid, or the autoregressive point decoder itself return a word more than once.
 * utils/overlap.py holds the specification (coverage_cpu, pair_overlap_cpu, suppress_cpu); every output integer equals it.
 *   polys       int32 [n][32]: 16 points (x0, y0, ..., x15, y15) in coordinate bins, the polygon decoder's tokens; every coordinate is
 *               CLAMPED on the device to [0, grid - 1]; 2 <= grid <= 4096
 *   coverage    a polygon covers the bin centres (i + 0.5, j + 0.5), 0 <= i, j < grid - 1, inside it under the even-odd rule, decided in
 *               doubled integer coordinates (vertices even, samples odd): edge (x1, y1) -> (x2, y2), oriented so that q = y2 - y1 > 0,
 *               counts for sample (xs, ys) when (y1 < ys) != (y2 < ys) and xs q < x1 q + (ys - y1) (x2 - x1)
 *   group_start int32 [n_groups + 1]: polygons group_start[g] .. group_start[g + 1] - 1 form group g (an image); only polygons of one
 *               group interact; entries are clamped into [0, n] on the device.  A group holds at most 8192 polygons.
 *   order       int32 [n]: the priority order, grouped like the polygons: order[group_start[g] + p] is the polygon at priority position p
 *               of group g (a global index, clamped into the group on the device)
 *   t, measure  permille threshold 1 .. 1000 and 0 = IoU / 1 = intersection over the smaller area: b overlaps a when inter > 0 and
 *               1000 inter >= t (area_a + area_b - inter), resp. >= t min(area_a, area_b); 64-bit products
 *   mask_start  int64 [n_groups + 1]: group g's bitmask begins at word mask_start[g] and holds n_g rows of W_g = ceil(n_g / 64) words;
 *               mask_start[n_groups] = mask_words (at most 2^32)
 * Outputs, all written by the call (the caller initialises nothing):
 *   area  int32 [n]: samples inside each polygon;  bbox int32 [n][4]: x0, y0, x1, y1 of the clamped points
 *   mask  uint64 [mask_words]: row p, bit q (word q / 64, bit q % 64) is set when q > p and the polygons at priority positions p and
 *         q overlap; every other bit is 0
 *   inter int32 [inter_total] or NULL: group g's dense n_g x n_g matrix at inter_start[g] (int64 [n_groups + 1]), in POLYGON order,
 *         inter[a][b] = samples inside both, the diagonal = area.  With NULL the area-ratio prefilter also applies.
 * Two launches (a wave per polygon; a wave per mask word); no allocation, no synchronisation. */
int omp_polygon_overlap(const int32_t* polys, int n, const int32_t* group_start, int n_groups, const int32_t* order,
                        const int64_t* mask_start, int64_t mask_words, int grid, int t, int measure, int32_t* area, int32_t* bbox,
                        uint64_t* mask, int32_t* inter, const int64_t* inter_start, int64_t inter_total, omp_stream_t s);
/* Greedy suppression over omp_polygon_overlap's mask: walk each group's positions in priority order; a polygon is kept unless an
 * earlier kept polygon overlaps it.  owner int32 [n]: the polygon itself when kept, else the first kept polygon, in priority order,
 * that overlaps it.  kept int32 [n_groups]: polygons kept per group; -1 for a group that is REFUSED on the device (more than 8192
 * polygons, or a mask range outside [0, mask_words)), whose owner entries are the polygons themselves.  One launch, one workgroup
 * per group. */
int omp_polygon_keep(const uint64_t* mask, const int64_t* mask_start, int64_t mask_words, const int32_t* group_start, int n_groups, int n,
                     const int32_t* order, int32_t* owner, int32_t* kept, omp_stream_t s);

/* ---- scoring: spotting results against ground truth under the IoU protocol ----
 * Neither reference project scores its results: engine/val.py writes a results JSON and stops.  utils/scoring.py holds the
 * specification (match_cpu, match_pages_cpu); this entry point equals it on every output integer.  Protocol: the polygons of image g
 * are ordered ground truth first (n_gt[g] of them), then detections; inter is omp_polygon_overlap's dense matrix of the group, so
 * area[p] = inter[p][p].  Detection d is ACTIVE at threshold index k iff level[d] > k.  Per (image, k):
 *   don't-care  an active detection d is don't-care when some ground-truth word i has gt_dc[i] != 0, inter[i][d] > 0 and
 *               1000 inter[i][d] >= t_dc area[d]
 *   matching    the ground-truth words i with gt_dc[i] == 0 are visited in index order; each takes the lowest-index detection d that
 *               is active, not don't-care, not yet taken, with inter[i][d] > 0 and 1000 inter[i][d] >= t_iou (area[i] + area[d] -
 *               inter[i][d]); 64-bit products.  A detection of area 0 never matches and is never don't-care.
 *   counts [n_groups][n_thr][4] = care ground truth, care detections (active and not don't-care), matched, matched with
 *               text[i] == text[d]
 * Inputs:
 *   inter        int32, group g's n_g x n_g matrix from inter_start[g] (int64 [n_groups + 1]; inter_start[n_groups] is the number of
 *                entries, which the caller guarantees the buffer holds)
 *   group_start  int32 [n_groups + 1], n_gt int32 [n_groups]; gt_dc, text, level int32 [n], indexed like the polygons (gt_dc is
 *                read at ground-truth rows only, level at detection rows only)
 *   n_thr 1 .. 64, t_iou and t_dc in permille 1 .. 1000, report -1 or a threshold index
 * Outputs: counts, written in full.  det_gt / gt_det int32 [n] (both or neither; needed when report >= 0), written in full: for
 *   k == report det_gt[d] = the matched ground-truth index inside the image, -1 care and unmatched, -2 don't-care, -3 inactive, at
 *   the detections' rows, and gt_det[i] = the matched detection's index among the image's detections, -1 unmatched, -2 don't-care, at
 *   the ground truth's rows; every other row, and every row when report is -1, holds -4.
 * OMP_ERR_INVALID, nothing launched: a null pointer (inter, gt_dc, text and level may be null when n is 0), n_groups < 1, n_thr, t_iou,
 *   t_dc or report outside their ranges.  The tables live in device memory, so what only they show is REFUSED on the device, as
 *   omp_polygon_keep does: an image of more than 8192 polygons, n_gt[g] outside 0 .. n_g, or a matrix outside the inter table gets
 *   counts of -1 (all n_thr x 4 of them) and -4 in its assignment rows, and reads nothing of inter.
 * One launch, a workgroup per (image, threshold); no allocation, no synchronisation. */
int omp_spotting_match(const int32_t* inter, const int64_t* inter_start, const int32_t* group_start, const int32_t* n_gt,
                       const int32_t* gt_dc, const int32_t* text, const int32_t* level, int n, int n_groups, int n_thr, int t_iou,
                       int t_dc, int report, int32_t* counts, int32_t* det_gt, int32_t* gt_det, omp_stream_t s);

/* ---- page text scoring: the Levenshtein distance of whole pages ----
 * The reference scores a parsed page as 1 - edit_distance(pred, gt) / max(len(pred), len(gt)) on strings without blanks and newlines
 * (Benchmarks/CC-OCR/evaluation/evaluator/doc_parsing_evaluator.py:223-238).  utils/page_text.py holds the specification (distance_cpu,
 * pairs_cpu); this entry point equals it on every integer.  Insert / delete / substitute cost 1.
 *   pool, pool_bytes   uint8 character codes: 0 .. sigma - 1, or 255, which equals nothing (itself included).  A code in sigma .. 254
 *                      is outside the contract and is treated like 255.
 *   a_off, a_len, b_off, b_len   int32 [n_pairs]: pair p is pool[a_off, a_off + a_len) against pool[b_off, b_off + b_len); ranges may
 *                      overlap and be shared between pairs.  Lengths 0 .. 65535.
 *   sigma              0 .. 254: the dynamic LDS of a workgroup is (sigma + 1) * 512 bytes
 *   scratch            8-byte aligned, at least n_pairs * 32768 bytes (pair p's carries between stripes of 4096 characters of a)
 *   dist               int32 [n_pairs], written in full
 * OMP_ERR_INVALID, nothing launched: a null pointer, n_pairs < 1, sigma outside 0 .. 254, too little scratch.  The tables live in
 *   device memory, so what only they show is REFUSED on the device: a pair with a negative length, a length above 65535 or a range
 *   outside the pool gets dist = -1 and reads nothing of the pool.
 * One launch, one wave per pair; no allocation, no synchronisation, no atomics. */
int omp_page_edit_distance(const uint8_t* pool, int64_t pool_bytes, const int32_t* a_off, const int32_t* a_len, const int32_t* b_off,
                           const int32_t* b_len, int n_pairs, int sigma, void* scratch, int64_t scratch_bytes, int32_t* dist,
                           omp_stream_t s);

/* ---- page search: fuzzy phrase matches in the text of read pages ----
 * Sellers' approximate string matching, insert / delete / substitute cost 1: D[0][j] = 0, D[i][0] = i, v_j = D[m][j].
 * utils/page_search.py holds the specification (row_cpu, search_cpu); this entry point equals it on every integer.
 *   pool, pool_bytes   uint8 character codes: 0 .. sigma - 1, or 255, which equals nothing (itself included).  A code in sigma .. 254
 *                      is outside the contract and is treated like 255.
 *   page_off, page_len int32 [n_pages]: page p is pool[page_off, page_off + page_len), 0 .. 65535 characters
 *   query_off, query_len, k   int32 [n_queries]: query q is pool[query_off, query_off + query_len), 1 .. 64 characters, with the
 *                      tolerance 0 <= k <= query_len - 1.  Ranges may overlap and be shared.
 *   jobs               int32 [n_jobs, 2]: (page, query); 1 .. 2^20 jobs
 *   max_hits           H, 1 .. 64
 *   scratch            8-byte aligned, at least n_jobs * 64 * max_hits * 8 bytes (per lane the first H hits of its chunk of the text)
 *   best               int32 [n_jobs, 2] = (dist, end): the least v_j and the least j that attains it; (m, 0) for the empty match
 *   n_hits             int32 [n_jobs]: the ends j in 1 .. n with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1})
 *   hits               int32 [n_jobs, H, 3] = (end, dist, start) of the first min(n_hits, H) hits in ascending end, the rest -1;
 *                      start is the greatest s with edit_distance(query, text[s, end)) == dist
 * OMP_ERR_INVALID, nothing launched: a null pointer, n_jobs outside 1 .. 2^20, no pages, no queries, sigma outside 0 .. 254, max_hits
 *   outside 1 .. 64, too little scratch.  The tables live in device memory, so what only they show is REFUSED on the device: a job
 *   whose page or query is not there, whose lengths are outside the limits, whose ranges lie outside the pool or whose k is outside
 *   0 .. m - 1 gets n_hits = -1 (best and hits -1) and reads nothing of the pool.
 * One launch, one wave per job; no allocation, no synchronisation, no atomics: the hits do not depend on scheduling. */
int omp_page_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                    const int32_t* query_off, const int32_t* query_len, const int32_t* k, int n_queries, const int32_t* jobs,
                    int n_jobs, int sigma, int max_hits, void* scratch, int64_t scratch_bytes, int32_t* best, int32_t* n_hits,
                    int32_t* hits, omp_stream_t s);

/* ---- page patterns: dates, amounts and ids in the text of read pages ----
 * A pattern is 1 .. 64 positions, each a character class, each mandatory or optional; insert / delete / substitute cost 1, skipping
 * an optional position is free: D[0][j] = 0, D[i][0] = D[i-1][0] + skip_i, D[i][j] = min(D[i-1][j-1] + (t_j not in C_i),
 * D[i-1][j] + skip_i, D[i][j-1] + 1), skip_i = 0 for an optional position and 1 otherwise; v_j = min(D[P][j], k + 1).
 * utils/page_pattern.py holds the specification (row_py, search_cpu); this entry point equals it on every integer.
 *   pool, pool_bytes   uint8 character codes 0 .. sigma - 1; a code at or above sigma is in no class
 *   page_off, page_len int32 [n_pages]: page p is pool[page_off, page_off + page_len), 0 .. 65535 characters
 *   masks              uint64 [n_patterns][sigma + 1], 8-byte aligned: bit i of masks[q][c] says that code c is in the class of position
 *                      i of pattern q; row sigma is not read (it counts as 0)
 *   opt, pat_len, k    uint64 / int32 / int32 [n_patterns]: bit i of opt says that position i is optional; P = pat_len in 1 .. 64, no opt
 *                      bit at or above P, Mand = P - popcount(opt) >= 1, and the tolerance 0 <= k <= min(Mand - 1, 8)
 *   jobs               int32 [n_jobs, 2]: (page, pattern); 1 .. 2^20 jobs
 *   max_hits           H, 1 .. 64
 *   scratch            8-byte aligned, at least n_jobs * 64 * max_hits * 8 bytes (per lane the first H hits of its chunk of the text)
 *   best               int32 [n_jobs, 2] = (dist, end): the least v_j and the least j that attains it; (k + 1, 0) when nothing is within k
 *   n_hits             int32 [n_jobs]: the ends j in 1 .. n with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1})
 *   hits               int32 [n_jobs, H, 3] = (end, dist, start) of the first min(n_hits, H) hits in ascending end, the rest -1;
 *                      start is the LEAST s >= end - (P + dist) whose anchored cost against text[s, end) equals dist (the longest match;
 *                      omp_page_search reports the shortest)
 * OMP_ERR_INVALID, nothing launched: a null pointer, n_jobs outside 1 .. 2^20, no pages, no patterns, sigma outside 0 .. 254, max_hits
 *   outside 1 .. 64, too little scratch, scratch, masks or opt not 8-byte aligned.  The tables live in device memory, so what only they
 *   show is REFUSED on the device: a job whose page or pattern is not there, whose P is outside 1 .. 64, whose opt word holds a bit at
 *   or above P or leaves no mandatory position, whose k is outside 0 .. min(Mand - 1, 8), whose page is above 65535 characters or lies
 *   outside the pool gets n_hits = -1 (best and hits -1) and reads nothing of the pool.
 * One launch, one wave per job; no allocation, no synchronisation, no atomics: the hits do not depend on scheduling. */
int omp_page_pattern_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                            const uint64_t* masks, const uint64_t* opt, const int32_t* pat_len, const int32_t* k, int n_patterns,
                            const int32_t* jobs, int n_jobs, int sigma, int max_hits, void* scratch, int64_t scratch_bytes, int32_t* best,
                            int32_t* n_hits, int32_t* hits, omp_stream_t s);

/* ---- page expressions: groups, alternation and real loops in the text of read pages ----
 * An expression is Glushkov's position automaton of P = 1 .. 64 positions, each a character class: first / last are the positions a
 * match can begin / end with, follow[i] the positions that can come after position i, pred is follow transposed.  Bit i of the state D
 * says that a match prefix has just consumed a character at position i: D_0 = 0, D_j = (Follow(D_{j-1}) | first) & masks[t_j] with
 * Follow(D) = OR of follow[i] over the bits i of D; column j (1-based) is an END iff D_j & last != 0.  The match is exact (no errors).
 * utils/page_regex.py holds the specification (ends_cpu, search_cpu); this entry point equals it on every integer.
 *   pool, pool_bytes   uint8 character codes 0 .. sigma - 1; a code at or above sigma is in no class
 *   page_off, page_len int32 [n_pages]: page p is pool[page_off, page_off + page_len), 0 .. 65535 characters
 *   masks              uint64 [n_expressions][sigma + 1], 8-byte aligned: bit i of masks[q][c] says that code c is in the class of
 *                      position i of expression q; row sigma is not read (it counts as 0)
 *   first, last        uint64 [n_expressions], neither 0, no bit at or above P
 *   follow, pred       uint64 [n_expressions][64]: no bit at or above P, the rows at or above P zero
 *   pat_len            int32 [n_expressions]: P in 1 .. 64
 *   jobs               int32 [n_jobs, 2]: (page, expression); 1 .. 2^20 jobs
 *   max_hits           H, 1 .. 64
 *   best               int32 [n_jobs, 2]: (0, the least end), or (1, 0) when the page holds no end
 *   n_hits             int32 [n_jobs]: the ends whose next column is no end (the LAST column of every run of consecutive ends)
 *   hits               int32 [n_jobs, H, 3] = (end, 0, start) of the first min(n_hits, H) hits in ascending end, the rest -1; start is
 *                      the LEAST s with text[s, end) in the language (the longest match), found by a walk back that has no span cap
 * OMP_ERR_INVALID, nothing launched: a null pointer, n_jobs outside 1 .. 2^20, no pages, no expressions, sigma outside 0 .. 254, max_hits
 *   outside 1 .. 64, masks, first, last, follow or pred not 8-byte aligned.  The tables live in device memory, so what only they show is
 *   REFUSED on the device: a job whose page or expression is not there, whose P is outside 1 .. 64, whose first, last, follow or pred
 *   words hold a bit or a row at or above P, whose first or last is 0, whose page is above 65535 characters or lies outside the pool
 *   gets n_hits = -1 (best and hits -1) and reads nothing of the pool.
 * One launch, one wave per job, no scratch; no allocation, no synchronisation, no atomics: the hits do not depend on scheduling. */
int omp_page_regex_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                          const uint64_t* masks, const uint64_t* first, const uint64_t* last, const uint64_t* follow, const uint64_t* pred,
                          const int32_t* pat_len, int n_expressions, const int32_t* jobs, int n_jobs, int sigma, int max_hits, int32_t* best,
                          int32_t* n_hits, int32_t* hits, omp_stream_t s);

/* ---- page expressions with errors: a regular expression within k edits in the text of read pages ----
 * The automaton and every table are omp_page_regex_search's; k holds one tolerance per expression.  Rows R_0 .. R_k, one 64-bit word each:
 * bit p of R_i after column j says that some text[s, j) aligns, with at most i insertions, deletions and substitutions of cost 1, to a
 * path of the automaton from first that ends at position p.  With Fol(X) = Follow(X) | first: before any text R_0 = 0, R_i = Fol(R_{i-1});
 * at column j with B = masks[t_j]: R'_0 = Fol(R_0) & B, R'_i = (Fol(R_i) & B) | Fol(R_{i-1}) | R_{i-1} | Fol(R'_{i-1}).  v_j is the least
 * i with R'_i & last != 0, else k + 1; v_0 = k + 1.  utils/page_regex.py holds the specification (dist_cpu, fuzzy_start,
 * fuzzy_search_cpu); this entry point equals it on every integer.
 *   pool .. pat_len, jobs, max_hits   as omp_page_regex_search takes them
 *   k                  int32 [n_expressions]: 0 .. 4.  The caller keeps k below the length of the expression's shortest word (the host
 *                      side checks it); the kernel does not need it
 *   best               int32 [n_jobs, 2]: (the least v_j, the least column that attains it), or (k + 1, 0) when nothing is within k
 *   n_hits             int32 [n_jobs]: the columns with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1})
 *   hits               int32 [n_jobs, H, 3] = (end, dist, start) of the first min(n_hits, H) hits in ascending end, the rest -1; start is
 *                      the LEAST s whose anchored distance of text[s, end) to the language equals dist, found by a walk back without a cap
 * OMP_ERR_INVALID, nothing launched: as omp_page_regex_search, and a null k.  REFUSED on the device (n_hits = -1, best and hits -1, nothing
 *   of the pool read): everything omp_page_regex_search refuses there, and a k outside 0 .. 4.
 * One launch, one wave per job, no scratch; no allocation, no synchronisation, no atomics: the hits do not depend on scheduling. */
int omp_page_regex_fuzzy_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                                const uint64_t* masks, const uint64_t* first, const uint64_t* last, const uint64_t* follow, const uint64_t* pred,
                                const int32_t* pat_len, const int32_t* k, int n_expressions, const int32_t* jobs, int n_jobs, int sigma,
                                int max_hits, int32_t* best, int32_t* n_hits, int32_t* hits, omp_stream_t s);

/* ---- page text alignment: the optimal edit script of whole pages ----
 * The script behind omp_page_edit_distance's number: a is the prediction (rows i), b the ground truth (columns j), D the Levenshtein
 * table with D[i][0] = i and D[0][j] = j.  The walk runs from (la, lb) to (0, 0) and takes the FIRST rule that applies:
 *   1. i > 0, j > 0, D[i-1][j-1] + (a_i != b_j) == D[i][j]: MATCH or SUB, a_map[i-1] = j-1, b_map[j-1] = i-1
 *   2. i > 0, D[i-1][j] + 1 == D[i][j]: INS, a_map[i-1] = -1            3. otherwise DEL, b_map[j-1] = -1
 * utils/page_align.py holds the specification (align_cpu, pairs_align_cpu); this entry point equals it on every integer.
 *   pool, pool_bytes   uint8 character codes, as omp_page_edit_distance takes them (255 equals nothing, itself included)
 *   a_off, a_len, b_off, b_len   int32 [n_pairs]: pair p is pool[a_off, a_off + a_len) against pool[b_off, b_off + b_len); ranges may
 *                      overlap and be shared between pairs.  Lengths 0 .. 65535.
 *   map_off            int64 [n_pairs]: pair p owns maps[map_off, map_off + a_len + b_len), a_map first and b_map after it
 *   scratch_off        int64 [n_pairs], multiples of 8: pair p owns 32768 + 16 * ceil(a_len / 64) * b_len bytes of scratch from there
 *                      (the carries between stripes, then per 64-row block and text column two 64-bit words: diagonal allowed, dv = +1)
 *   sigma              0 .. 254: the dynamic LDS of a workgroup is (sigma + 1) * 512 bytes
 *   scratch            8-byte aligned, scratch_bytes bytes; the slices of two pairs must not overlap
 *   maps, maps_len     int32 [maps_len]; entries no pair owns are left as they are
 *   counts             int32 [n_pairs][4] = (match, sub, ins, del), written in full; sub + ins + del is the distance
 * OMP_ERR_INVALID, nothing launched: a null pointer, n_pairs outside 1 .. 2^24, sigma outside 0 .. 254, pool_bytes, maps_len or
 *   scratch_bytes negative, scratch not 8-byte aligned.  The tables live in device memory, so what only they show is REFUSED on the
 *   device: a pair with a negative length, a length above 65535, a range outside the pool, a negative map_off or a slice past maps_len,
 *   a scratch_off that is negative or no multiple of 8, or a slice past scratch_bytes gets counts = -1 four times, reads nothing of
 *   the pool and writes nothing to maps or scratch.
 * One launch, one wave per pair; no allocation, no synchronisation, no atomics: the script does not depend on scheduling. */
int omp_page_align(const uint8_t* pool, int64_t pool_bytes, const int32_t* a_off, const int32_t* a_len, const int32_t* b_off,
                   const int32_t* b_len, const int64_t* map_off, const int64_t* scratch_off, int n_pairs, int sigma, void* scratch,
                   int64_t scratch_bytes, int32_t* maps, int64_t maps_len, int32_t* counts, omp_stream_t s);

/* ---- reading order: words -> text lines -> the order a reader takes them in ----
 * Neither reference project orders its words: they leave the engine in decoder order.  utils/reading.py holds the specification
 * (features_cpu, links_cpu, lines_cpu); every output integer equals it.  Integers only.
 *   polys       int32 [n][32], 16-byte aligned: 16 points in coordinate bins, CLAMPED on the device to [0, grid - 1]; 2 <= grid <= 4096
 *   tables      device int32 [3 n_groups + 1]: group_start [n_groups + 1] (words group_start[g] .. group_start[g + 1] - 1 are image g's;
 *               only words of one group interact), then aspect [n_groups][2] = (ax, ay), 1 .. 256: geometry is done on (x ax, y ay)
 *   host_tables the same int32 [3 n_groups + 1] in HOST memory: checked before anything is launched (group_start rises from 0 to n,
 *               every aspect in 1 .. 256); the device clamps what it reads all the same
 *   gap, back, offset  permille, 0 .. 10000
 *   features    T[k] = P[k], B[k] = P[15 - k]; L = T[0] + B[0], R = T[7] + B[7], d = R - L ((1, 0) when 0), H = sum_k |(T[k] - B[k]) x d|
 *   link a -> b with v = L_b - R_a: d_a . d_b > 0, -back H_a <= 4000 v . d_a <= gap H_a, 4000 |v x d_a| <= offset H_a,
 *               4000 |v x d_b| <= offset H_b; cost = |v|^2 (below 2^46)
 * omp_reading_links: succ0 int32 [n] = the passing b of least cost (ties to the lower b; a global index) or -1, cost0 int64 [n] = its
 * cost or -1.  One launch: workgroups of 256 words inside one group, candidates staged through LDS in tiles of 256.
 * n == 0 returns OMP_OK without a launch. */
int omp_reading_links(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid, int gap, int back,
                      int offset, int32_t* succ0, int64_t* cost0, omp_stream_t s);
/* Lines from omp_reading_links' candidates, one workgroup per group, everything in LDS: a word claimed by several keeps the
 * predecessor of least (cost, a) and the losers end their lines; a cycle is cut in front of its lowest member; lines are ordered by
 * the mean of their members' sum_k y_k ay (compared exactly), then the head's L_x, then the head's index.
 *   succ, pred  int32 [n]: global indices, -1 at a line's ends;  line, line_pos, rank int32 [n]: the line's number in its group, the
 *               distance from the line's head, the position in the group with the lines concatenated
 *   n_lines     int32 [n_groups]: lines per group; -1 for a group that is REFUSED on the device (more than 8192 words), of whose
 *               words nothing is written
 * One launch.  n == 0 returns OMP_OK without a launch. */
int omp_reading_lines(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid,
                      const int32_t* succ0, const int64_t* cost0, int32_t* succ, int32_t* pred, int32_t* line, int32_t* line_pos,
                      int32_t* rank, int32_t* n_lines, omp_stream_t s);
/* Blocks: a recursive XY-cut over omp_reading_lines' lines, for multi-column pages.  Neither reference project has
 * layout analysis; utils/reading.py::blocks_cpu is the specification and every output integer equals it.  Stands for: blocks_cpu.
 *   gap_x, gap_y  permille of a word's height, 0 .. 10000; depth 1 .. 16: the number of levels at most
 *   line_in, line_pos_in int32 [n], n_lines_in int32 [n_groups]: omp_reading_lines' line, line_pos and n_lines, on the device
 *   per word, on the scaled points: the bounding box, s = sum_k (B[k] - T[k]), t = max(|s_x|, |s_y|), the inflated intervals
 *               [16000 x0 - gap_x t, 16000 x1 + gap_x t] and the same on y with gap_y (below 2^38 in magnitude); a line's interval is the
 *               min / max over its words.  Level l cuts y (l even) or x (l odd): inside every segment, in (lo, line) order, a line starts
 *               a new component when its lo is strictly greater than the largest hi in front of it; components numbered in (segment,
 *               position) order are the new segments.  Stops after depth levels or after two levels in a row that created none.
 *   block, line, rank int32 [n]: the word's block in its group (reading order from 0), its line renumbered through the blocks, its
 *               position with the lines concatenated in the new order;  n_blocks, levels int32 [n_groups]: blocks per group and levels
 *               run (0, 0 for a group without words); n_blocks = -1 for a group that is REFUSED on the device (more than 8192 words),
 *               of which nothing else is written
 * One launch, one workgroup of 1024 threads per group, everything in LDS (a bitonic sort and scans per level); no allocation and no
 * synchronisation.  n == 0 returns OMP_OK without a launch. */
int omp_reading_blocks(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid, int gap_x,
                       int gap_y, int depth, const int32_t* line_in, const int32_t* line_pos_in, const int32_t* n_lines_in, int32_t* block,
                       int32_t* line, int32_t* rank, int32_t* n_blocks, int32_t* levels, omp_stream_t s);

/* ---- tiled pages: the words of overlapping full-resolution tiles -> the words of their pages ----
 * Neither reference project reads a page in tiles: both scale it to the model's input size.  utils/tiles.py::remap_cpu is the
 * specification and every output integer equals it.  Integers only.
 *   polys, points  int32 [n][32], [n][2]: the decoders' ids in TILE bins, every one CLAMPED on the device to [0, nb - 1]; 2 <= nb <= 4096
 *   tables      device int32 [6 n_tiles + 1 + 2 n_pages] = row_start [n_tiles + 1] (words row_start[k] .. row_start[k + 1] - 1 are tile
 *               k's) | tile_rect [n_tiles][4] (x0, y0, x1, y1 in page pixels, x1 / y1 exclusive) | tile_page [n_tiles] | page_size
 *               [n_pages][2] (W, H; 1 .. 65535)
 *   remapping   an x id c of a tile [x0, x1) on a page of width W -> min(P - 1, (2 (x0 nb + c (x1 - x0)) P + nb W) / (2 nb W)), P =
 *               page_bins (2 .. 4096), in 64 bits; y with y0, y1 and H
 *   cut bits    from the clamped ids of the word's 17 points: 1 x0 > 0 and min x <= edge; 2 y0 > 0 and min y <= edge; 4 x1 < W and
 *               max x >= nb - 1 - edge; 8 y1 < H and max y >= nb - 1 - edge (0 <= edge <= 4096)
 *   refusals    a tile whose row range is not 0 <= row_start[k] <= row_start[k + 1] <= n, whose page is outside the table or not 1 ..
 *               65535 pixels a side, or whose rectangle is empty or leaves its page is REFUSED on the device: tile_count -1,
 *               tile_dropped 0, and nothing else of it is written
 * Outputs, all int32; everything but cut and scratch is written in full by the call:
 *   scratch [n][34]  working space: the remapped row of every word of an accepted tile
 *   cut [n]          the cut bits of the words of accepted tiles; the entries of other words are NOT written (ops.tile_remap
 *                    initialises them to -1, which is what the specification gives them)
 *   page_polys [cap][32], page_points [cap][2], src_row [cap]: the remapped rows and the word indices of the words with cut == 0 (of
 *                    all words of accepted tiles when drop_cut is 0), in tile order and inside a tile in the decoder's order (a stable
 *                    compaction); entries at or beyond cap are not written (out_start[n_tiles] still holds the full total)
 *   tile_count, tile_dropped [n_tiles]: words kept / removed per tile;  out_start [n_tiles + 1]: exclusive prefix sum of the kept
 *                    counts;  page_count [n_pages]: words kept per page (through tile_page)
 * Three launches (flag, scan, copy); no allocation, no synchronisation. */
int omp_tile_remap(const int32_t* polys, const int32_t* points, int n, const int32_t* tables, int n_tiles, int n_pages, int nb,
                   int page_bins, int edge, int drop_cut, int32_t* scratch, int32_t* cut, int32_t* page_polys, int32_t* page_points,
                   int32_t* src_row, int cap, int32_t* tile_count, int32_t* tile_dropped, int32_t* out_start, int32_t* page_count,
                   omp_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* OMP355_H */
