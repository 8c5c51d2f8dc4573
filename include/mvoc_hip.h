/*
 * libmvoc_hip.so -- C ABI of the MI355X (gfx950) kernels behind MVOC's denoising hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes, is asynchronous on the HIP
 * stream passed as `void* stream` (a hipStream_t), never allocates or frees device memory, never
 * synchronises the device and keeps no pointer past return (graph-capture safe).  Return value: 0 on
 * success, -1 invalid argument, -2 unsupported shape, -3 HIP error; text via mvoc_last_error()
 * (thread-local).  The caller (PyTorch) owns all buffers.  fp16 = IEEE binary16.
 *
 * Canonical activation layout in HBM: channels-last "tokens" [B, F, H*W, C] (row-major, C contiguous),
 * i.e. a [rows = B*F*H*W, C] matrix.  Spatial ops see it as [B*F images][H*W][C]; temporal ops walk
 * the frame axis with row stride H*W.  The reference's NCHW <-> token <-> frame-major permute copies
 * (pnp_utils.py:185-189, 207-213, 434-437, 502-506) do not exist here.
 *
 * Each entry names the reference interface it replaces (paths relative to the reference checkout).
 */
#ifndef MVOC_HIP_H
#define MVOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVOC_VERSION 100

int mvoc_version(void);
const char* mvoc_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM on MFMA (fp16 in, fp32 accumulate, fp16 out):  out[m, n] = epi( sum_k A(m,k) * W[n,k] )
 * Replaces every F.linear / F.conv2d(3x3, 1x1) / F.conv3d((3,1,1)) on the path:
 *   F.linear  pnp_utils.py:191,206,438,505,604-612,692,759-767,870; pipeline_i2vgen_xl.py:188,193,231
 *   conv2d    pnp_utils.py:939,968,1013 (ResnetBlock2D), :1112 (conv_out); pipeline_i2vgen_xl.py:284
 *   conv3d    pnp_utils.py:1048-1051 (TemporalConvLayer)
 * ------------------------------------------------------------------------------------------- */
enum { MVOC_A_PLAIN = 0, MVOC_A_CONV3X3 = 1, MVOC_A_TEMPORAL3 = 2 };
enum { MVOC_ACT_NONE = 0, MVOC_ACT_GEGLU = 1, MVOC_ACT_SILU = 2, MVOC_ACT_GELU = 3 };

typedef struct mvoc_gemm_desc {
  /* operands */
  const void* a;        /* activation source 1 (fp16) */
  const void* a2;       /* optional source 2 for a channel-concat input (cat([x, skip], dim=1)); NULL if none */
  const void* w;        /* weights [n][k] fp16 (upsample == 2: [4 n][k]), k contiguous, no row beyond n is needed; for conv k = tap*cin + c
                           (tap-major; k_order = 1: chunk-major, below) */
  void* out;            /* [m][ldo] fp16 */
  const void* bias;     /* [n] fp16 or NULL (GEGLU: packed like w rows) */
  const void* rowadd;   /* optional [m / rowadd_div][ld_rowadd] fp16 added per output row (time embedding) */
  const void* resid;    /* optional residual [m][ldr] fp16 added after bias/act */
  int64_t m, n, k;      /* n = rows of w (multiple of 32); k multiple of 32 */
  int32_t n_store;      /* columns actually written (<= n; GEGLU: n/2) */
  int32_t ldo, ldr, ld_rowadd, rowadd_div;
  int32_t a_mode;       /* MVOC_A_* */
  int32_t lda, lda2;    /* row strides (elements) of a / a2 */
  int32_t c1;           /* channels taken from `a` per tap (rest from a2); == cin when a2 == NULL */
  int32_t cin;          /* conv / temporal: channels per tap (c1 + c2); plain: == k */
  /* conv3x3 (pad 1): output pixel grid [nimg][hout][wout]; source image [hsrc][wsrc]; if upsample != 0 the
   * conv runs on the nearest-upsampled [hup][wup] view of the source (Upsample2D folded into the gather).
   * upsample == 2: the SUB-PIXEL form of an exact 2x upsample (hup == 2 hsrc, wup == 2 wsrc): the three taps of a row of the 3 x 3
   * kernel fall on only two source rows (columns likewise), so per output parity (a, b) the conv is a 2 x 2 conv on the source
   * image -- 4 taps of matrix work instead of 9.  `w` then holds the four parity kernels [4 = 2 a + b][n][dy][dx][cin] (k = 4 cin,
   * tap (dy, dx) of parity a: dy = 0 <- ky 0, dy = 1 <- ky 1 + ky 2 for a = 0; dy = 0 <- ky 0 + ky 1, dy = 1 <- ky 2 for a = 1; columns
   * likewise: mvoc_amd.unet.pack_conv3x3_subpixel) and the source pixel (i, j) of parity (a, b) is output pixel (2 i + a, 2 j + b).
   * Plain epilogue (bias) only, one source, nimg hsrc wsrc a multiple of 256, no split-K, no chan_sums. */
  int32_t nimg, hout, wout, hsrc, wsrc, stride, upsample, hup, wup;
  /* temporal3 (pad 1 over frames): rows are [nvid][frames][hw] */
  int32_t frames, hw;
  int32_t act;          /* MVOC_ACT_* */
  int32_t tile;         /* 0 = auto; otherwise force a tile config id (tuning) */
  int32_t split_k;      /* 0 = auto, 1 = off, n = force n K-slices (needs workspace; direct-to-LDS tiles only) */
  void* workspace;      /* optional fp32 scratch for split-K partial slabs: split_k * m * n * 4 bytes */
  size_t workspace_bytes;
  /* LayerNorm folded into the GEMM (F.layer_norm feeding F.linear at pnp_utils.py:250/296/322 -> :604-612, :335):
   * `a` holds the RAW rows, `w` holds gamma-scaled weights W' = W * gamma; the epilogue forms
   * rstd*(acc - mean*ln_rowsum[n]) + ln_bias[n] with the rows' {mean, rstd} from `ln_stats` (REQUIRED in this mode).
   * ln_rowsum = sum_k W'[n,k], ln_bias = beta @ W^T + bias, both fp32 [n]; `bias` is ignored in this mode.  NULL = off. */
  const void* ln_rowsum;
  const void* ln_bias;
  float ln_eps;
  int32_t pad_mode;     /* conv3x3: 0 = zero padding 1 on every side (F.conv2d(padding=1)); 1 = one row / column of zeros at the
                           BOTTOM / RIGHT only (F.pad(x, (0,1,0,1)) + conv2d(padding=0, stride=2): the downsamplers of the VAE
                           encoder, diffusers Downsample2D(padding=0)) */
  const void* ln_stats; /* {mean, rstd} per row, fp32 [m][2], from mvoc_row_stats_f16 (two-pass variance, one read of the rows, shared
                           by every n-tile) or mvoc_row_stats_from_moments_f32.  REQUIRED with ln_rowsum: the GEMM kernels take no
                           row statistics themselves. */
  void* chan_sums;      /* optional REQUEST, fp32 [m / 256][n_store][2] (honoured only when m is a multiple of 256): per 256-row slab
                           and output channel, the sum and the
                           sum of squares of the values this call stores (fp16-rounded, residual included) -- the first pass of the
                           GroupNorm that reads `out` next (F.group_norm at pnp_utils.py:909-910, 953-965, 1048-1051, 185-188),
                           taken from the producer's epilogue instead of a separate read of the tensor.  Written only when the
                           launch runs on the eight-phase tiles without split-K and without activation: ask
                           mvoc_gemm_chan_sums_written() after the call; when it answers 0 the buffer is untouched and the
                           consumer computes its own statistics (mvoc_groupnorm_f16 without chan_sums).  These are ONE-PASS moments per
                           slab (fp32-exact products summed in fp32); the consumers form M2 = sumsq - sum * mean per slab and channel
                           group and Chan-merge the slabs, so cancellation is bounded by one slab's |mean| / sigma (as row_moments
                           below: 2e-3 relative on rstd at |mean| / sigma = 150, far from this network's activations). */
  void* row_moments;    /* optional REQUEST, fp32 [m][row_moments_ld][2]: per output ROW and n-tile of the launch, the sum and the sum of
                           squares of the values this call stores over the tile's channels -- the statistics of the LayerNorm that
                           reads `out` next (F.layer_norm at pnp_utils.py:250-257, 296, 322), taken from the producer's epilogue
                           instead of a pass over the tensor (mvoc_row_stats_f16).  Written only by the eight-phase tiles without
                           split-K and with n_store == n: ask mvoc_gemm_row_moments_written() after the call -- 0: untouched;
                           otherwise the tile width w (256 or 320): entry [r][t] covers channels [t w, min(n, (t + 1) w)), and
                           mvoc_row_stats_from_moments_f32 turns the entries of a row into its {mean, rstd}. */
  int32_t row_moments_ld; /* entries per row of row_moments: >= ceil(n / 256) */
  int32_t concurrency;  /* scheduling hint, 0 / 1 = the launch has the chip to itself: the caller runs this many independent launches of
                           this shape at the same time on other streams (the job's per-object inversions, inverse.py:136-190, as
                           concurrent loops), so an under-filled grid need not be split over K to fill the chip.  Clamped to 8.  It
                           changes the tile / split-K choice, hence the summation order of a launch (results differ from the unhinted
                           launch by fp16 rounding of another order, never by more); per call, no process-wide state. */
  int32_t k_order;      /* conv3x3 / temporal3 only.  0: `w` is tap-major, k = tap * cin + c (above).  1: CHANNEL-CHUNK-major with the taps
                           innermost, k = (c / 64) * (ntaps * 64) + tap * 64 + c % 64 (ntaps = 9 / 3; mvoc_amd.ops.chunk_major_weights):
                           the nine (three) taps of one 64-channel slab of the source are consumed back to back, so the re-reads a block
                           makes of its own pixel rows (each source line is read once per tap: F.conv2d at pnp_utils.py:939, 968, conv3d at
                           :1042-1057) are ~50 KB apart instead of a whole tap's cin * 256 rows and hit the XCD's L2.  Same products, same
                           fp32 sums in another order (exact on integer operands).  A form of the 320-WIDE eight-phase tile (it runs on that
                           tile whatever `tile` says): n a multiple of 320, cin, c1 multiples of 64, conv stride 1 / pad 1 on a
                           same-size source or temporal3, no upsample, no activation, no LayerNorm fold, no split-K, m >= 1024, 16-byte
                           addressable operands < 2 GB: anything else is an error (-2), not a fall-back -- the caller holds the
                           tap-major weights for those launches. */
} mvoc_gemm_desc;

/* Extents (enforced by tests/test_gemm_contract_gpu.py on every tile id, on allocations whose undescribed elements are NaN; cols =
 * n_store, or n where n_store is 0, GEGLU: n / 2; rows_a = nimg hsrc wsrc for conv3x3, else m):
 *   - only these elements influence a result: a[rows_a][c1] at pitch lda and a2[rows_a][cin - c1] at pitch lda2 (plain: cin = k),
 *     w[n][k] (upsample == 2: [4 n][k]), bias[n], rowadd[ceil(m / rowadd_div)][cols] at pitch ld_rowadd, resid[m][cols] at pitch ldr,
 *     ln_rowsum[n], ln_bias[n], ln_stats[m][2].  The columns of a / a2 at and past c1 / cin - c1 (the column views taken of fused
 *     projections), the residual's and the row-add's columns at and past cols and the gaps between their rows, whatever lies around
 *     any operand, and the prior contents of the workspace never do, whatever they hold;
 *   - conv3x3 with k > 9 cin (the K of the small-channel convs, padded to a multiple of 32): the columns of w at and past 9 cin ARE
 *     described and must hold zeros, as mvoc_amd.unet.pack_conv3x3 writes them: the kernels zero the activation side there and still
 *     multiply, so a NaN or an infinity in them reaches the result;
 *   - no byte of out outside [m][cols] at pitch ldo is written, no byte of the workspace past split_k * m * n * 4, and none of the
 *     input operands;
 *   - chan_sums and row_moments: either the query function below answers non-zero and exactly [m / 256][cols][2], respectively the
 *     entries [m][ceil(n / w)][2] of rows of row_moments_ld entries, are written (the further entries of a row are not), or it
 *     answers 0 and no byte of the operand is written.  After a call that returns non-zero both answer 0;
 *   - the return value is always one of 0, -1, -2, -3 (top of this file), with the text in mvoc_last_error(); a refused call
 *     writes nothing. */
int mvoc_gemm_f16(const mvoc_gemm_desc* d, void* stream);
/* 1 when this thread's most recent mvoc_gemm_f16 call wrote its descriptor's chan_sums */
int mvoc_gemm_chan_sums_written(void);
/* tile width (256 / 320) when this thread's most recent mvoc_gemm_f16 call wrote its descriptor's row_moments, else 0 */
int mvoc_gemm_row_moments_written(void);
/* {mean, rstd} per row (fp32 [rows][2], the layout of mvoc_row_stats_f16 / ln_stats) from a producer's row_moments: the n-tiles'
 * {sum, sum of squares} become {count, mean, M2} per tile and are Chan-merged in tile order. */
int mvoc_row_stats_from_moments_f32(const void* moments, int64_t rows, int32_t ld, int32_t n, int32_t tile_w, float eps,
                                    void* out_stats, void* stream);
/* scratch for the deterministic split-K form of a launch: the most the auto policy uses is 8 slices of m*n fp32
 * partials; 0 when the policy would never split this shape (m > 8192 or k < 2048).  Passing no workspace is always valid:
 * the launch then runs unsplit. */
size_t mvoc_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k);

/* ---------------------------------------------------------------------------------------------
 * Attention, head_dim 64, softmax(Q K^T / 8) V, no mask (F.scaled_dot_product_attention at
 * pnp_utils.py:684-686, 862-864 and the stock AttnProcessor2_0 sites).
 * q/k/v/out element (b, t, h, d) lives at base + b*bs + t*ts + h*head_dim + d  (elements).
 * kv batch index = b / kv_bdiv (cross-attention context shared by all frames of a sample).
 * The descriptor describes exactly the elements (b, t, h, d) with b < nbatch (b / kv_bdiv for k / v / v2), t < tq (q, out, out2) or
 * t < tk (k, v, v2), h < heads, d < head_dim: elements outside these extents (padding rows behind a batch entry's last row, columns
 * of a row beyond heads * head_dim, whatever follows the last row) never influence a result, whatever they hold, and no byte of
 * out / out2 outside the described extents is written.  (tests/test_attention_contract_gpu.py fills them with NaN / a sentinel.)
 * The fields from head_dim on are optional: a caller that does not use them must leave them ZERO (zero-initialise the whole
 * descriptor, e.g. `mvoc_attn_desc d = {0};`): an uninitialised head_dim / causal / scale / v2 / out2 / pipelined is read as a request.
 * ------------------------------------------------------------------------------------------- */
typedef struct mvoc_attn_desc {
  const void *q, *k, *v;
  void* out;
  int64_t q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts;
  int32_t nbatch, heads, tq, tk, kv_bdiv;
  /* the three below default (0) to the UNet's form: head_dim 64, no mask, scale 1/8.  head_dim 96 with scale 1/sqrt(80)
   * serves CLIP ViT-H's 80-wide heads (projection weights zero-padded per head); causal: key <= query (CLIP text tower,
   * pipeline_i2vgen_xl.py:552-737 encode_prompt -> CLIPTextModel) */
  int32_t head_dim, causal;
  float scale;
  /* paired form (head_dim 64): a second value tensor / output with the layout of v / out that attends with the SAME q and k --
   * the PnP destination chunks after Q/K injection (pnp_utils.py:664-668 assigns one blended q / k to both the unconditional and
   * the conditional chunk; only their v differ).  NULL: plain attention.  Results equal two plain calls bit for bit. */
  const void* v2;
  void* out2;
  /* kernel choice of THIS call (head_dim 64, no causal mask): 0 by key count (the software-pipelined kernel from 2 048 keys up), 1 the
   * phase kernel always, 2 the pipelined kernel wherever it applies.  Speed only -- both kernels return the same bits (the tests
   * compare them).  Replaces round 4's process-wide setter (flash_pipelined): the library keeps no mutable state between calls
   * (MVOC_FLASH3=0|1 in the environment changes the default of 0 at load time, for diagnostics). */
  int32_t pipelined;
} mvoc_attn_desc;

/* spatial self-attention and image/text cross-attention (flash-style, K/V tiles LDS-staged) */
int mvoc_flash_attn_f16(const mvoc_attn_desc* d, void* stream);
/* temporal self-attention: one sequence per (sample, pixel), tq == tk == frames <= 32; "t" walks frames
 * (ts = H*W*C for the canonical layout), "b" walks sample*pixel via (b / hw)*bs + (b % hw)*ps.
 * Described are the elements (sample < nsample, pixel < hw, frame < frames, h < heads, d < 64) of each operand: elements outside
 * these extents (padding pixels, frames or columns between them, whatever follows the last) never influence a result, whatever they
 * hold, and no byte of out outside the described extents is written.  Every field is required; a descriptor that grows trailing
 * optional fields is to be zero-initialised as a whole (`mvoc_tattn_desc d = {0};`), as for mvoc_attn_desc. */
typedef struct mvoc_tattn_desc {
  const void *q, *k, *v;
  void* out;
  int64_t q_bs, q_ps, q_ts, k_bs, k_ps, k_ts, v_bs, v_ps, v_ts, o_bs, o_ps, o_ts;
  int32_t nsample, hw, heads, frames;
} mvoc_tattn_desc;
int mvoc_temporal_attn_f16(const mvoc_tattn_desc* d, void* stream);

/* Activation-stationary linear for K in {64, 128, 320} (the 320-channel level's projections: F.linear at pnp_utils.py:191, 206,
 * 335, 438, 505, 604-612, 692): out[m][n] = epi(x[m][:] . W[n][:] + c[n]).  A wave keeps 32 consecutive rows of x in registers;
 * the weights AND the per-channel constants stream through LDS from a packed copy (mvoc_amd.unet.pack_xs_weights):
 *   wp [n/32 tiles][k/16 + 1 pieces][lane < 64][8 fp16]
 *      piece s < k/16: element = W[32 tile + (lane & 31)][16 s + 8 (lane >> 5) + j]  (MFMA fragment order)
 *      piece k/16    : its first 128 bytes are the tile's 32 constants c[32 tile + i] as fp32 (bias, or beta @ W^T + bias)
 * normalize != 0 folds a LayerNorm in front (rows normalised in registers; W must be gamma-scaled, c = beta @ W^T + bias).
 * act as for mvoc_gemm_f16 (GEGLU: weight rows in (value, gate) blocks of 32, n/2 outputs, no residual).  x is [m][k]
 * contiguous; out / resid rows 16-byte addressable per 8 channels; n_store may only trim the last 32-channel tile.
 * Extents (enforced by tests/test_xs_contract_gpu.py on allocations whose undescribed elements are NaN; cols = n_store, or
 * n (GEGLU: n / 2) where n_store is 0):
 *   - only the elements x[m][k], the wp stream(s) ((m / wp_set_rows, or 1) x n/32 tiles x (k/16 + 1) KB), of each tile's
 *     constants piece its first 128 bytes, and resid[m][cols] at pitch ldr influence a result: the other 896 bytes of a
 *     constants piece, the residual's columns >= cols and the gaps between its rows, and whatever lies around x, wp and resid
 *     never do, whatever they hold;
 *   - no byte of out outside [m][cols] at pitch ldo is written;
 *   - x and wp must be 16-byte aligned (both are read in 16-byte pieces); a misaligned pointer is refused with -2. */
typedef struct mvoc_xs_desc {
  const void* x;
  const void* wp;
  const void* resid;
  void* out;
  int64_t m;
  int32_t n, k, n_store, ldo, ldr, act, normalize;
  float ln_eps;
  int64_t wp_set_rows;  /* 0: one weight stream for every row.  > 0: `wp` holds m / wp_set_rows consecutive streams, set j for rows
                           [j wp_set_rows, (j + 1) wp_set_rows) -- the per-sample weights of a folded GroupNorm
                           (mvoc_groupnorm_fold_xs_f16); a multiple of 256 */
} mvoc_xs_desc;
int mvoc_xs_linear_f16(const mvoc_xs_desc* d, void* stream);


/* Fused front half of a temporal self-attention at the finest level: LayerNorm -> to_q/to_k/to_v -> attention over the frame
 * axis, Q/K/V never written to HBM (TransformerTemporalModel's attn1 / attn2: pnp_utils.py:170-220, 222-346, 720-887; replaces
 * mvoc_row_stats_f16 + the fused-QKV mvoc_gemm_f16 + mvoc_temporal_attn_f16 where no PnP Q/K injection is scheduled).
 *   x   [nsample*frames*hw][c] raw rows of the canonical layout (c = heads*64 in {64, 128, 320}, frames in {8, 16, 32})
 *   wp  the gamma-scaled [3c][c] projection W' = cat(Wq, Wk, Wv) * gamma re-ordered in MFMA fragment order:
 *       [head][tile: q0 k0 q1 k1 v0 v1][k16 step s < c/16][lane < 64][8 fp16], element = W'[row0 + (lane & 31)][16 s + 8 (lane >> 5) + j]
 *       with row0 = 64 head + {0, c, 32, c + 32, 2c, 2c + 32}[tile]   (mvoc_amd.unet.pack_tfused_weights)
 *   ln_rowsum / ln_bias fp32 [3c] as for the folded GEMM; out [rows][c] = heads concatenated, before to_out
 * Extents (enforced by tests/test_tfused_contract_gpu.py on allocations whose undescribed elements are NaN; rows =
 * nsample * frames * hw):
 *   - only the elements x[rows][c], wp[3c * c], ln_rowsum[3c] and ln_bias[3c] influence a result (the rows are normalised in
 *     registers, so ln_rowsum is not even read; it stays in the contract because the unfused chain needs it): whatever lies
 *     around them never does, whatever it holds;
 *   - every element of out[rows][c] is written and no byte outside it is;
 *   - x, wp and out must be 16-byte aligned (x and wp are read, out is written in 16-byte pieces), ln_rowsum and ln_bias 4-byte
 *     aligned; a misaligned pointer is refused with -2, and so is nsample > 65535 (the sample index is a grid dimension).  A
 *     refused call launches nothing;
 *   - ln_eps is honoured as given (the variance is that of the row, eps is added to it before the reciprocal square root). */
typedef struct mvoc_tfused_desc {
  const void* x;
  const void* wp;
  const void* ln_rowsum;
  const void* ln_bias;
  void* out;
  int32_t nsample, frames, hw, c, heads;
  float ln_eps;
} mvoc_tfused_desc;
int mvoc_temporal_qkv_attn_f16(const mvoc_tfused_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm (+SiLU) on channels-last rows; F.group_norm + F.silu at pnp_utils.py:909-910, 953-965 (4-D,
 * statistics per image), :188 and TemporalConvLayer (5-D, statistics per video), :430, and
 * pipeline_i2vgen_xl.py:351-352.  Input may be a 2-source channel concat.  Deterministic (no atomics).
 *   workspace floats: nsample * (nchunk*3 + 2) * groups  -> mvoc_groupnorm_workspace_bytes
 * Extents (every entry of this family, mvoc_row_stats_f16, mvoc_layernorm_f16 and mvoc_row_stats_from_moments_f32 included;
 * enforced by tests/test_norm_contract_gpu.py on allocations whose undescribed elements are NaN):
 *   - only the elements [nsample * rows_per_sample][c1] of x and [..][c - c1] of x2 influence a result; likewise only the
 *     described extents of gamma, beta, chan_sums(2), parts and moments, and of a moments row of stride ld only its
 *     ceil(n / tile_w) tile entries;
 *   - no byte of out, stats, moments or wp_sets outside its extent is written;
 *   - no byte of the workspace beyond mvoc_groupnorm_workspace_bytes(...) is written;
 *   - the workspace's prior contents never influence a result.
 * ------------------------------------------------------------------------------------------- */
typedef struct mvoc_gn_desc {
  const void* x;        /* [nsample*rows_per_sample][c1] fp16 */
  const void* x2;       /* optional second source [..][c - c1] */
  const void* gamma;    /* [c] fp16 */
  const void* beta;     /* [c] fp16 */
  void* out;            /* [nsample*rows_per_sample][c] fp16 */
  void* workspace;
  size_t workspace_bytes;
  int32_t nsample, rows_per_sample, c, c1, groups, silu;
  float eps;
  /* optional: the statistics pass taken from the producers of x (and x2): what mvoc_gemm_f16 wrote into its descriptor's
   * chan_sums when it stored these rows -- fp32 [nsample * rows_per_sample / 256][c1][2] (and [..][c - c1][2]).  Needs
   * rows_per_sample % 256 == 0 and c1 % (c / groups) == 0; both sources' sums when x2 is given.  NULL: the statistics are
   * read from x. */
  const void* chan_sums;
  const void* chan_sums2;
} mvoc_gn_desc;
size_t mvoc_groupnorm_workspace_bytes(int32_t nsample, int32_t rows_per_sample, int32_t c, int32_t groups);
int mvoc_groupnorm_f16(const mvoc_gn_desc* d, void* stream);
/* GroupNorm folded into the linear that reads it (GN -> proj_in, no activation in between: pnp_utils.py:185-191, 433-438):
 * takes the statistics of d's rows as mvoc_groupnorm_f16 does (d->x, nsample, rows_per_sample, c, groups, eps, gamma, beta,
 * workspace, chan_sums; single source; d->out unused) and writes, per SAMPLE, the weight stream of
 * mvoc_xs_linear_f16 for W'_s = W gamma rstd_s and c'_s = bias + W (beta - gamma mean_s rstd_s): wp_sets
 * [nsample][n / 32][k / 16 + 1][512] fp16.  The consumer then runs on the RAW rows with wp_set_rows = rows_per_sample; the
 * normalised tensor is never written.  w [n][k] fp16 row-major (k == c), bias [n] fp16 or NULL. */
int mvoc_groupnorm_fold_xs_f16(const mvoc_gn_desc* d, const void* w, const void* bias, int32_t n, int32_t k, void* wp_sets,
                               void* stream);

/* The same GroupNorm in two halves, for a sample whose rows are spread over several GPUs (frame-axis shard of one
 * long clip, SURVEY 8e / BASELINE configs[3]: the 5-D norms at pnp_utils.py:185-188 and inside TemporalConvLayer,
 * pnp_utils.py:1048-1051, take their statistics over ALL frames and pixels):
 *   moments : this rank's rows -> moments [nsample][groups][3] fp32 {count, mean, M2}   (gamma/beta/out unused)
 *   exchange: the caller all-gathers the triples (RCCL; 12*nsample*groups bytes per rank) -> parts [nparts][nsample][groups][3]
 *   apply   : Chan-combines the parts in index order (every rank gets bit-identical mean/rstd) and normalises this rank's rows.
 * With nparts == 1 the pair reproduces mvoc_groupnorm_f16 bit for bit. */
int mvoc_groupnorm_moments_f16(const mvoc_gn_desc* d, void* moments, void* stream);
int mvoc_groupnorm_apply_moments_f16(const mvoc_gn_desc* d, const void* parts, int32_t nparts, void* stream);

/* per-row {mean, rstd} (fp32 [rows][2]) of a [rows, c] fp16 matrix: the statistics half of F.layer_norm for GEMMs that
 * fold the normalisation into their epilogue (mvoc_gemm_desc.ln_*) */
/* c % 8 == 0, c <= 2048 (a row lives in one wave's registers: 4 x 16 bytes per lane) */
int mvoc_row_stats_f16(const void* x, void* stats, int64_t rows, int32_t c, float eps, void* stream);

/* LayerNorm over the last dim (F.layer_norm at pnp_utils.py:250,296,322), eps 1e-5, affine */
int mvoc_layernorm_f16(const void* x, const void* gamma, const void* beta, void* out, int64_t rows, int32_t c,
                       float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PnP masked blend + scatter.  For every (frame f, pixel p, channel c):
 *     inj = base;  for j in objects:  inj = inj*(1-m_j) + obj_j*m_j     (three fp16-rounded ops, in this order)
 *     chunk[n-2] = chunk[n-1] = inj
 * with chunks positional [bg, obj_1..obj_k, uncond, cond] (k <= 4; the reference hard-codes k = 2, n = 5:
 * pnp_utils.py:592,747,784,972,1061,1115), base = chunk n-1 (or chunk 0 when
 * base_chunk0 != 0), m_j = mask_j[f, nearest(p)] (fp16 values: exact {0,1} for bool masks, k/255 for soft masks).
 * BIT-EXACT against the reference arithmetic (not a select: -0.0 / inf / NaN propagate as in x*(1-m)+y*m).
 *   tokens: element (chunk, f, p, c) at x + chunk*chunk_stride + f*f_stride + p*p_stride + c   (c contiguous)
 *           -> spatial Q/K [5F, HW, C]   (pnp_utils.py:624-672):  chunk_stride=F*HW*C, f_stride=HW*C, p_stride=C
 *           -> temporal Q/K [5HW, F, C]  (pnp_utils.py:778-850):  chunk_stride=HW*F*C, f_stride=C,    p_stride=F*C
 *           -> canonical [5, F, HW, C] features (resnet / temporal-conv / conv_out injection)
 *   nchw:   x [5F, C, H, W] (pnp_utils.py:970-1004, 1059-1082, 1114-1146): p contiguous
 * masks: [nobj][F][mh][mw] fp16, nearest-resized to (H, W) like F.interpolate(mode='nearest').
 * Up to two tensors (Q and K) are processed by one launch (x2 may be NULL).
 * Alignment: the tokens entries read and write 16-byte vectors and return -2 with an error text (nothing launched) unless x
 * and x2 are 16-byte aligned (channels and the three strides are multiples of 8 already); the nchw entries take any 2-byte
 * aligned x / x2 and run 8 pixels per work item when H*W is a multiple of 8 and both pointers are 16-byte aligned, else one.
 * Masks need 2-byte and tables 4-byte alignment.
 * ------------------------------------------------------------------------------------------- */
typedef struct mvoc_pnp_desc {
  void* x;
  void* x2;
  const void* masks;
  int64_t chunk_stride, f_stride, p_stride;
  int32_t nobj, frames, height, width, channels, mask_h, mask_w, base_chunk0;
  /* base_chunk0: 0 = the base is the last chunk, 1 = the base is chunk 0 (the layouts above).  -1 = NO BACKGROUND CHUNK:
     the tensors hold [obj_1..obj_k, (uncond,) cond] -- object j (counted from 0) is chunk j, the chunk count is k + ndst and the
     base is the last chunk; arithmetic and object order are unchanged, so the destination rows are bit-identical to base_chunk0 = 0
     on the layout with a background chunk in front (which that blend never reads).  Taken by the positional
     mvoc_pnp_blend_scatter_tokens only: every _nchw entry and every entry that takes a map returns -1 with an error text and
     launches nothing (a map expresses the layout already: nsrc = k, obj_chunk[j] = j, base_chunk0 = 0; the feature blends of
     the _nchw entries need chunk 0).  A zero-initialised descriptor means what it always meant. */
  int32_t ndst;  /* trailing destination chunks: 0 or 2 = [uncond, cond] (the reference's layout), 1 = [cond] only: the
                    classifier-free-guidance-off batch [bg, obj_1..obj_k, cond] (n = k + 2) */
} mvoc_pnp_desc;
int mvoc_pnp_blend_scatter_tokens(const mvoc_pnp_desc* d, void* stream);
int mvoc_pnp_blend_scatter_nchw(const mvoc_pnp_desc* d, void* stream);
/* Source de-duplication (pipeline.py dedup_sources): roles that are the same source share one chunk, the batch is
 * [s_0..s_{nsrc-1}, uncond, cond] (or [s_0..s_{nsrc-1}, cond] with ndst = 1).  Chunk 0 is the background's, object j reads
 * chunk obj_chunk[j] (a HOST array of d->nobj entries, read during the call only: the map travels in the kernel arguments,
 * so a captured graph replays it), the destination chunks start at nsrc and the base is chunk 0, or the last chunk when
 * base_chunk0 == 0.  Same arithmetic and object order as above: the destination rows are bit-identical to the unmapped
 * entry on the sources expanded back to nobj + 1 chunks.  Requires 1 <= nsrc <= nobj + 1 and 0 <= obj_chunk[j] < nsrc
 * (else -1 and an error text). */
int mvoc_pnp_blend_scatter_tokens_mapped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, void* stream);
int mvoc_pnp_blend_scatter_nchw_mapped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, void* stream);
/* K variants over one set of sources (pipeline.py variants): nvar destination pairs share the source chunks, the
 * batch is [s_0..s_{nsrc-1}, u_1..u_K, c_1..c_K] (ndst = 1: [s_0..s_{nsrc-1}, c_1..c_K]); nsrc / obj_chunk as above (the
 * identity map {1..nobj} with nsrc = nobj + 1 is the positional source layout).  Every work item reads its nobj object vectors
 * and mask values once; variant k blends them onto chunk 0 (base_chunk0 != 0: one blend, stored ndst*K times) or onto its own
 * conditional chunk c_k, and stores to u_k and c_k (c_k only with ndst = 1).  The destination rows of variant k are
 * bit-identical to the positional entry on that variant's own [bg, obj.., u_k, c_k] batch; nvar = 1 is the _mapped entry.
 * Traffic per tensor: (distinct sources read + K bases when base_chunk0 == 0) + ndst*K chunks written.
 * Requires 1 <= nvar <= 8 and a valid map (else -1 and an error text, nothing written). */
int mvoc_pnp_blend_scatter_tokens_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                           void* stream);
int mvoc_pnp_blend_scatter_nchw_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                         void* stream);
/* Per-variant injection schedules: the _variants entries with a bitmask -- bit k of `active` set = variant k
 * injects at this launch.  An injecting variant's u_k / c_k rows are what the _variants entry writes; the chunks of every other
 * variant are neither read nor written.  `active` travels by value in the kernel arguments (no device array: a captured graph
 * replays it).  Traffic per tensor: distinct sources read (+ popcount(active) bases when base_chunk0 == 0) +
 * ndst * popcount(active) chunks written.
 * Requires 1 <= nvar <= 8, 1 <= active < (1u << nvar) and a valid map (else -1 and an error text, nothing written). */
int mvoc_pnp_blend_scatter_tokens_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                               uint32_t active, void* stream);
int mvoc_pnp_blend_scatter_nchw_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                             uint32_t active, void* stream);
/* Placement: the _variants_sel entries with a per-frame integer translation of every object -- here nvar = 1 and
 * every bit of `active` set are allowed too.  `place` is a DEVICE table of int32 pairs [nobj][frames][2] = (dfy, dfx), the
 * feature offsets of object j in frame f on THIS call's height x width grid; the caller owns it and keeps it unchanged for as
 * long as a captured graph may replay the launch.  For destination pixel (py, px) of frame f object j contributes the vector of
 * its chunk at pixel (py - dfy, px - dfx) of frame f and the mask value masks[j][f][nearest(py)][nearest(px)] -- the masks are
 * given in DESTINATION coordinates (mvoc_shift_planes_f16 moves them there) and sampled at the destination pixel as above.
 * Where the source pixel lies outside the frame the object is absent: value 0 and mask 0 enter the same three fp16-rounded ops
 * (nothing is skipped: a -0.0 base becomes +0.0 as under a zero mask).  The destination rows are bit-identical to the entries
 * above on object chunks shifted with zero fill and masks zeroed where the source is out of range; a table of zeros is the
 * _variants_sel entry.  Same traffic as _variants_sel.  Every int32 offset is valid (an object may leave the frame entirely);
 * the table's contents are on the device and are not read by the host.
 * Requires a non-NULL table, 1 <= nvar <= 8, 1 <= active < (1u << nvar) and a valid map (else -1 and an error text, nothing
 * written). */
int mvoc_pnp_blend_scatter_tokens_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                         uint32_t active, const int32_t* place, void* stream);
int mvoc_pnp_blend_scatter_nchw_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                       uint32_t active, const int32_t* place, void* stream);
/* Per-variant placement: the _placed entries with an offset table and masks PER VARIANT.  `place` is a DEVICE
 * table of int32 pairs [nvar][nobj][frames][2] = (dfy, dfx) for this call's height x width; variant k reads object j of frame f
 * at (py - dfy, px - dfx) taken from row (k * nobj + j) * frames + f.  d->masks points at [nvar][nobj][frames][mask_h][mask_w]:
 * variant k's masks in ITS destination coordinates, sampled at the destination pixel by the nearest rule above.  Absent objects,
 * the 64-bit source pixel, the three fp16-rounded ops per object, object order, ndst, base_chunk0, the source map and `active`
 * are those of _placed; the chunks of a variant whose bit is clear are neither read nor written.  With base_chunk0 != 0 the base
 * vector is loaded once per work item and every injecting variant blends it with its own objects.  Variant k's destination
 * rows are bit-identical to the _placed entry with nvar = 1 on that variant's own [sources.., (u_k,) c_k] batch with table k
 * and masks k; nvar = 1 is the _placed entry, nvar equal tables with equal masks are the _placed entry with that table.
 * Bytes counted per launch (MvocProfScope), with on = popcount(active), E = frames*height*width*channels, T = tensors (1 or 2):
 *     T * (2*E * (on * distinct object chunks + (base_chunk0 ? 1 : on) + ndst * on) + 2 * on * nobj*frames*height*width)
 *       + 8 * nvar*nobj*frames
 * i.e. each injecting variant reads its objects at its own pixels and one mask value per object and pixel, the base is read
 * once when it is chunk 0 and once per injecting variant otherwise, ndst * on chunks are written, and the table is read.
 * Requires a non-NULL table, 1 <= nvar <= 8, 1 <= active < (1u << nvar) and a valid map (else -1 and an error text, nothing
 * written). */
int mvoc_pnp_blend_scatter_tokens_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                  uint32_t active, const int32_t* place, void* stream);
int mvoc_pnp_blend_scatter_nchw_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                uint32_t active, const int32_t* place, void* stream);
/* Zero-filled per-frame integer translation of contiguous fp16 planes [nplane][frames][h][w] (src != dst):
 *     dst[pl][f][y][x] = src[pl][f][y - dy_f][x - dx_f], or 0 where that pixel lies outside the plane
 * `offsets`: DEVICE int32 pairs [frames][2] = (dy_f, dx_f), shared by the nplane planes -- the planes of one call belong to one
 * object: one [F][h][w] mask of a [nobj, F, h, w] stack per call (nplane = 1), or the four channels of an object's
 * [4, F, h, w] latents (nplane = 4).  Every int32 offset is valid. */
int mvoc_shift_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                          const int32_t* offsets, void* stream);
/* Scale and mirror: the _placed entries with a nearest-neighbour GATHER in place of the shift.  `maps` is a DEVICE
 * table of int32 [nobj][frames][height + width]: row (j * frames + f) holds ymap (height entries) and then xmap (width entries)
 * of object j in frame f on THIS call's height x width grid; the caller owns it and keeps it unchanged for as long as a captured
 * graph may replay the launch.  For destination pixel (py, px) of frame f object j contributes the vector of its chunk at pixel
 * (ymap[py], xmap[px]) of frame f and the mask value masks[j][f][nearest(py)][nearest(px)] -- the masks are given in DESTINATION
 * coordinates (mvoc_gather_planes_f16 moves them there) and sampled at the destination pixel as above.  An entry outside
 * [0, height) / [0, width) -- -1 by convention, but EVERY int32 value is safe: the entries are compared unsigned and the source
 * pixel is formed in 64 bits -- means the object is absent there: value 0 and mask 0 enter the same three fp16-rounded ops
 * (nothing is skipped: a -0.0 base becomes +0.0 as under a zero mask).  Object order, ndst, base_chunk0, the source map, nvar and
 * `active` are those of _placed.  The destination rows are bit-identical to the entries above on object chunks gathered with
 * zero fill and masks zeroed where a map entry is outside; maps ymap[y] = y - dfy, xmap[x] = x - dfx are the _placed entry with
 * the table (dfy, dfx), identity maps the _variants_sel entry.  Bytes counted per launch (MvocProfScope): those of _placed
 * + 4 * nobj*frames*(height + width) for the table.  The table's contents are on the device and are not read by the host.
 * Requires a non-NULL table, 1 <= nvar <= 8, 1 <= active < (1u << nvar), a valid map and base_chunk0 != -1 (else -1 and an error
 * text, nothing written). */
int mvoc_pnp_blend_scatter_tokens_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                            uint32_t active, const int32_t* maps, void* stream);
int mvoc_pnp_blend_scatter_nchw_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                          uint32_t active, const int32_t* maps, void* stream);
/* Per-variant transforms: the _resampled entries with a map table and masks PER VARIANT, in the shape of
 * _placed_variants.  `maps` is a DEVICE table of int32 [nvar][nobj][frames][height + width] (ymap, then xmap) for this call's
 * height x width; variant k reads object j of frame f at (ymap[py], xmap[px]) taken from row (k * nobj + j) * frames + f (the
 * row offset is formed in 64 bits).  d->masks points at [nvar][nobj][frames][mask_h][mask_w]: variant k's masks in ITS
 * destination coordinates.  Absent objects (every int32 entry is safe), the three fp16-rounded ops per object, object order,
 * ndst, base_chunk0, the source map and `active` are those of _resampled; the chunks of a variant whose bit is clear are neither
 * read nor written.  Variant k's destination rows are bit-identical to the _resampled entry with nvar = 1 on that variant's own
 * [sources.., (u_k,) c_k] batch with table k and masks k; nvar = 1 is the _resampled entry, translation-only tables are the
 * _placed_variants entry with the matching offsets.  Bytes counted per launch (MvocProfScope): the chunk and mask terms of
 * _placed_variants + 4 * nvar*nobj*frames*(height + width) for the table.
 * Requires a non-NULL table, 1 <= nvar <= 8, 1 <= active < (1u << nvar), a valid map and base_chunk0 != -1 (else -1 and an error
 * text, nothing written). */
int mvoc_pnp_blend_scatter_tokens_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                     uint32_t active, const int32_t* maps, void* stream);
int mvoc_pnp_blend_scatter_nchw_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                   uint32_t active, const int32_t* maps, void* stream);
/* Zero-filled per-frame gather of contiguous fp16 planes [nplane][frames][h][w] (src != dst):
 *     dst[pl][f][y][x] = src[pl][f][ymap_f[y]][xmap_f[x]], or 0 where either index lies outside the plane
 * `maps`: DEVICE int32 [frames][h + w], ymap_f (h entries) and then xmap_f (w entries), shared by the nplane planes (the planes
 * of one call belong to one object, as for mvoc_shift_planes_f16).  Every int32 entry is valid (compared unsigned). */
int mvoc_gather_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                           const int32_t* maps, void* stream);
/* Rotation: the _resampled entries with ONE 2-D index map in place of the two per-axis maps -- a rotation is not
 * separable.  `map` is a DEVICE table of int32 [nobj][frames][height * width] for THIS call's height x width: entry
 * (j * frames + f) * height * width + py * width + px is the linear source pixel sy * width + sx that object j of frame f
 * contributes to destination pixel (py, px); the caller owns the table and keeps it unchanged for as long as a captured graph may
 * replay the launch.  The object is present iff (uint32_t)entry < height * width -- -1 by convention, but EVERY int32 value is
 * safe: one unsigned compare takes the negative and the too-large entries alike.  Absent: value 0 and mask 0 enter the same
 * three fp16-rounded ops (nothing is skipped).  Masks (DESTINATION coordinates, mvoc_gather_planes_warped_f16 moves them there),
 * object order, ndst, base_chunk0, the source map, nvar and `active` are those of _resampled.  The destination rows are
 * bit-identical to the unplaced entries on object chunks gathered through the map with zero fill and masks zeroed where an entry
 * is outside; a map ymap[py] * width + xmap[px] (-1 where either is outside) is the _resampled entry with those per-axis maps.
 * The nchw entry reads the object values one pixel at a time; the base and the destinations are 16-byte vectors when
 * height * width is a multiple of 8 and x / x2 are 16-byte aligned.  Bytes counted per launch (MvocProfScope): those of _placed
 * + 4 * nobj*frames*height*width for the table.  The table's contents are on the device and are not read by the host.
 * Requires a non-NULL table, 1 <= nvar <= 8, 1 <= active < (1u << nvar), a valid source map and base_chunk0 != -1 (else -1 and an
 * error text, nothing written); height * width < 2^31 and, for tokens, the alignment rules of every tokens entry (else -2). */
int mvoc_pnp_blend_scatter_tokens_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                         uint32_t active, const int32_t* map, void* stream);
int mvoc_pnp_blend_scatter_nchw_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                       uint32_t active, const int32_t* map, void* stream);
/* Zero-filled per-frame gather of contiguous fp16 planes [nplane][frames][h][w] through a 2-D map (src != dst):
 *     dst[pl][f][y][x] = src[pl][f] at the linear pixel map_f[y * w + x], or 0 where that entry lies outside [0, h * w)
 * `map`: DEVICE int32 [frames][h * w], shared by the nplane planes (the planes of one call belong to one object, as for
 * mvoc_shift_planes_f16).  Every int32 entry is valid (compared unsigned).  Refuses what mvoc_gather_planes_f16 refuses. */
int mvoc_gather_planes_warped_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                  const int32_t* map, void* stream);
/* Bilinear sampling: the _warped entries with a TAP table in place of the 2-D map; the blend sites are those of the
 * family (pnp_utils.py:624-672, 778-850 for tokens; :970-1004, 1059-1082, 1114-1146 for nchw).  `taps` is a DEVICE table of int32
 * [nobj][frames][height * width][2] for THIS call's height x width; the pair of destination pixel (py, px) of object j, frame f is
 *     word 0 = ((y0 + 1) << 16) | (x0 + 1)    the upper-left tap, y0 in [-1, height - 1], x0 in [-1, width - 1]; -1 = absent
 *     word 1 = (qy << 16) | qx                weights in 1/256 of the LOWER row y0 + 1 and the RIGHT column x0 + 1 (9 bits are read)
 * The value of a tap (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) is used only if (uint32_t)row < height && (uint32_t)col <
 * width; a tap outside loads the plane's pixel 0 instead (always in bounds) and enters as +0.0: EVERY int32 pair is safe.  Value, one correctly rounded fp16 operation per statement, with
 * lerp(a, b, w0, w1) = r16(r16(a * w0) + r16(b * w1)) and fp16 weights wx1 = qx / 256, wx0 = (256 - qx) / 256 (same for y):
 *     top = lerp(v00, v01, wx0, wx1);  bot = lerp(v10, v11, wx0, wx1);  v = lerp(top, bot, wy0, wy1)
 * The object is present iff at least one tap lies inside the plane (a tap of weight 0 counts); absent: value 0 and mask 0 enter
 * the same three fp16-rounded blend ops (nothing is skipped).  A tap inside the plane is multiplied even with weight 0 (inf in a
 * source gives NaN), and -0.0 leaves the chain as +0.0.  Masks (DESTINATION coordinates), object order, ndst, base_chunk0, the
 * source map, nvar and `active` are those of _warped.  The destination rows are bit-identical to the unplaced entries on object
 * chunks interpolated beforehand by this chain, with masks zeroed where the object is absent; a table with q = 0 everywhere is
 * the _warped entry with the map y0 * width + x0 (for sources without -0.0).  Bytes counted per launch (MvocProfScope): those of
 * _placed (each distinct object chunk once) + 8 * nobj*frames*height*width for the table.  The table's contents are on the device
 * and are not read by the host.  The caller owns the table and keeps it unchanged while a captured graph may replay the launch.
 * Requires what _warped requires (-1 / -2 and an error text, nothing written) and height, width < 65535 (else -2). */
int mvoc_pnp_blend_scatter_tokens_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                           uint32_t active, const int32_t* taps, void* stream);
int mvoc_pnp_blend_scatter_nchw_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                         uint32_t active, const int32_t* taps, void* stream);
/* Zero-filled per-frame bilinear gather of contiguous fp16 planes [nplane][frames][h][w] (src != dst): dst[pl][f][y][x] = the
 * chain above on the four taps of taps_f[y * w + x] read from src[pl][f], 0 where no tap lies inside the plane.  `taps`: DEVICE
 * int32 [frames][h * w][2], shared by the nplane planes.  Every int32 pair is valid.  Refuses what mvoc_gather_planes_warped_f16
 * refuses, and h or w >= 65535 (-2). */
int mvoc_gather_planes_bilinear_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                    const int32_t* taps, void* stream);

/* The main conditioning frames of a composition: the background with every object alpha-blended over it, sampled
 * through a tap table at the IMAGE site, in integers only.  bg uint8 [frames][h][w][3], objs uint8 [nobj][frames][h][w][3], alpha
 * uint8 [nobj][frames][h][w] (straight alpha, 0..255), out uint8 [frames][h][w][3], all contiguous on the device; `taps`: DEVICE
 * int32 [nobj][frames][h * w][2], 8-byte aligned (an entry is read as one int2), in the form above: word 0 names the upper-left tap,
 * -1 where absent; of word 1's two 9-bit weight fields a value above 256 counts as 256.  That clamp is this entry's alone -- the fp16
 * entries above read the 9 bits as they are and do not clamp, so the two decodings agree for q <= 256, which is every table the
 * builders make; here it keeps every sample a byte and all arithmetic inside int32 for ANY table.  Per pixel and channel, o = bg; for j = 0 .. nobj-1 (later objects in front), with
 *   S(v) = ((v00*(256-qx) + v01*qx)*(256-qy) + (v10*(256-qx) + v11*qx)*qy + 32768) >> 16    (a tap outside the plane: 0)
 *   a = S(alpha_j);  o = (o*(255-a) + S(objs_j)*a + 127) / 255
 * A tap outside the plane issues its loads at the plane's pixel 0 and is masked to 0: every int32 pair is valid.  Reports
 * frames*h*w * (6 + 12*nobj) bytes (MVOC_FAM_MISC).  Refuses, in this order, with nothing written: a null operand (-1), out equal
 * to an input (-1), nobj outside [1, 16] or a non-positive dim (-1), h or w >= 65535 (-2), h * w >= 2^31 (-2), a grid too large (-2). */
int mvoc_collage_rgb_u8(const void* bg, const void* objs, const void* alpha, void* out, int32_t nobj, int32_t frames, int32_t h,
                        int32_t w, const int32_t* taps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Matte edges at composition time: one PASS of the grow / shrink / feather filter over src[nplane][h][w], written to
 * dst[nplane][h][w], fp16 (the latent masks) or uint8 (the image-size alphas), both contiguous, no alignment beyond the element.
 * A pass filters every plane along one axis (axis 0: along y, 1: along x) with the window 2*radius + 1.  Tap indices are clamped to
 * the plane (replicated border), so a plane never reads its neighbour; with i the position on the axis and v the line,
 *   op 0 max  : o = v[clamp(i-radius)]; for d = -radius+1 .. radius: t = v[clamp(i+d)]; if (t > o) o = t      (exact in either type)
 *   op 1 min  : the same with t < o
 *   op 2 mean : fp16: acc = 0.0f; for d = -radius .. radius in this order: acc += (float)v[clamp(i+d)];  o = (half)(acc * inv),
 *                     inv = (float)(1.0 / (2*radius + 1)) formed by the caller in double and rounded once to float
 *               u8  : o = (2*sum + n) / (2*n) with n = 2*radius + 1, in int32, floor
 * radius 0 is a copy.  An edit of a mask is max or min along x, then along y (grow, shrink), then the mean along x, then along y
 * (feather), the intermediate stored in the plane's own type (mvoc_amd.ops.edit_planes).  Only src[nplane][h][w] is read and only
 * dst[nplane][h][w] is written, whatever lies around them.  One work item per element, 256 per block, 64-bit element index.
 * Reports 2 * nplane*h*w * sizeof(element) bytes (MVOC_FAM_MISC).  Returns 0, -3 (launch failure) or refuses, in this order, with
 * nothing written and the text in mvoc_last_error: a null operand (-1), src == dst (-1), a non-positive dim (-1), op outside 0..2
 * or axis outside 0..1 (-1), radius outside [0, 64] (-2), h * w >= 2^31 (-2), a grid too large (-2). */
int mvoc_mask_filter_f16(const void* src, void* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, int32_t radius,
                         int32_t axis, float inv, void* stream);
int mvoc_mask_filter_u8(const void* src, void* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, int32_t radius,
                        int32_t axis, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loop glue on [B,4,F,h,w] fp16 latents, BIT-EXACT vs the reference's eager fp16 op chain.
 *   cfg + DDIM / inverse-DDIM update (pipeline_i2vgen_xl.py:1187-1199, 1713-1731, 1967-1984;
 *   diffusers DDIMScheduler.step / DDIMInverseScheduler.step, v_prediction, eta = 0):
 *     v   = uncond + g*(cond-uncond)            (skipped when uncond == NULL: v = cond)
 *     x0  = sa*x - sb*v ; eps = sa*v + sb*x ; out = sp*x0 + sq*eps
 *   coef = {sa, sb, sp, sq, g} fp32 on the DEVICE (so a captured graph can be replayed per step)
 * ------------------------------------------------------------------------------------------- */
int mvoc_ddim_step_f16(const void* x, const void* v_uncond, const void* v_cond, const float* coef_dev, void* out,
                       int64_t n, void* stream);
/* latent noise fusion (pipeline_i2vgen_xl.py:1644-1663); objs/masks: nobj device pointers packed in arrays
 * of contiguous [n] fp16 tensors: obj[j] at objs + j*n, mask[j] at masks + j*n */
int mvoc_latent_fusion_f16(const void* latents, const void* bg, const void* objs, const void* masks, void* out,
                           int32_t nobj, int64_t n, double mix_ratio, int32_t obj_random_noise_fusion, void* stream);
/* The two updates over K variants in one launch (1 <= nvar <= 8), bit-identical variant by variant to the entries above.
 *   ddim_step:     x / v_uncond / v_cond / out are [nvar][n_per]; coef_dev is [nvar][5], element i uses row i / n_per
 *   latent_fusion: latents / out are [nvar][n_per]; bg [n_per], objs / masks [nobj][n_per] are read by every variant */
int mvoc_ddim_step_variants_f16(const void* x, const void* v_uncond, const void* v_cond, const float* coef_dev, void* out,
                                int64_t n_per, int32_t nvar, void* stream);
int mvoc_latent_fusion_variants_f16(const void* latents, const void* bg, const void* objs, const void* masks, void* out,
                                    int32_t nobj, int64_t n_per, int32_t nvar, double mix_ratio,
                                    int32_t obj_random_noise_fusion, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stem / small ops (pipeline_i2vgen_xl.py:166-290, 351-357).
 *
 * Extents (enforced by tests/test_stem_contract_gpu.py for the nineteen entries of this section, of the VAE, mask and CLIP sections
 * below and mvoc_permute_rows_f16: one thread per output, walked at 1, 255, 256, 257 and 513 work items on allocations whose
 * undescribed elements are NaN).  Common to all of them:
 *   - only the elements named per entry influence a result; the columns of a pitched row past its c channels, a table the form does
 *     not index, and whatever lies around any operand never do, whatever they hold;
 *   - no byte outside the described output is written: not the other channels of an ldo- or ld-pitched row (columns below coff and at
 *     or past coff + c keep what they held), nothing in front of or behind the operand, and no input operand;
 *   - operands need the alignment of their element (2 bytes fp16, 4 bytes fp32 / int32) unless the entry says 16 bytes;
 *   - the return value is 0, -1 (a NULL operand, a non-positive extent, or the precondition the entry names) or -3 (launch failure),
 *     with the text in mvoc_last_error(); a refused call launches nothing and writes nothing.
 * Per entry:
 *   timestep_embedding  reads t[nb] (fp32); writes out[nb][dim], out[b][k] = cos, out[b][dim/2 + k] = sin of t[b] * 10000^(-k / (dim/2)),
 *                       evaluated in fp32 and rounded once.  -1: dim odd.
 *   act                 reads x[n], writes out[n]: act = MVOC_ACT_SILU x / (1 + exp(-x)), MVOC_ACT_GELU 0.5 x (1 + erf(x / sqrt 2)), in
 *                       fp32, rounded once (within one fp16 ulp of the fp64 value, GELU plus 2^-22 |x|).
 *   add                 reads a[n], b[n], writes out[n]: the exact sum rounded once.
 *   conv3x3_small       reads x[nimg][h][wd][cin], w[cout][3][3][cin], bias[cout] (NULL: none); writes out[nimg][ho][wo][cout], ho =
 *                       (h - 1) / stride + 1, wo likewise; the tap (ky, kx) of output (oy, ox) is x[oy stride + ky - 1][ox stride + kx - 1],
 *                       zero outside the image; fp32 sum + bias rounded to fp16, then SiLU (silu != 0) rounded again.  -1: stride not 1 or 2.
 *   adaptive_avgpool    reads x[nimg][h][w][c], writes out[nimg][oh][ow][c]: the mean over rows [floor(oy h / oh), ceil((oy + 1) h / oh))
 *                       and the columns likewise (torch's AdaptiveAvgPool2d windows; oh > h repeats rows): fp32 sum / fp32 count, rounded once.
 *   ncfhw_to_tokens     reads x[b][c][f][hw]; writes out[b f hw][ldo] in the columns [coff, coff + c) only.  -1: coff < 0, ldo < coff + c.
 *   tokens_to_ncfhw     reads x[b f hw][ld] in the columns [0, c) only; writes out[b][c][f][hw].  -1: ld < c.
 *   temporal_encoder4   reads x[b f hw][4] and the 288 fp16 of params; writes out[b f hw][ldo] in the columns [coff, coff + 4) only; the row
 *                       of pixel (bi, p), frame i depends on the f rows x[bi][.][p] alone.  Rounded to fp16 after the LayerNorm, each of
 *                       q / k / v, the attention output, to_out + bias, the residual sum, FF1 + bias, GELU, FF2 + bias and the last sum
 *                       (softmax and sums in fp32).  -1: coff < 0, ldo < coff + 4.
 * ------------------------------------------------------------------------------------------- */
/* sinusoidal Timesteps(dim, flip_sin_to_cos=True, shift 0): out[b] = [cos | sin] rounded to fp16; t fp32 on device */
int mvoc_timestep_embedding_f16(const float* t_dev, int32_t nb, int32_t dim, void* out, void* stream);
/* y = silu(x) / gelu(x) elementwise, fp16 */
int mvoc_act_f16(const void* x, void* out, int64_t n, int32_t act, void* stream);
/* out = a + b (fp16, rounded once) */
int mvoc_add_f16(const void* a, const void* b, void* out, int64_t n, void* stream);
/* direct 3x3 conv (pad 1) on channels-last images for tiny channel counts; w [cout][3][3][cin] fp16 */
int mvoc_conv3x3_small_f16(const void* x, const void* w, const void* bias, void* out, int32_t nimg, int32_t h,
                           int32_t wd, int32_t cin, int32_t cout, int32_t stride, int32_t silu, void* stream);
/* AdaptiveAvgPool2d on channels-last images */
int mvoc_adaptive_avgpool_f16(const void* x, void* out, int32_t nimg, int32_t h, int32_t w, int32_t c, int32_t oh,
                              int32_t ow, void* stream);
/* [B,C,F,h,w] (reference boundary layout) -> channels-last [B,F,h*w,ldo] at channel offset coff */
int mvoc_ncfhw_to_tokens_f16(const void* x, void* out, int32_t b, int32_t c, int32_t f, int32_t hw, int32_t ldo,
                             int32_t coff, void* stream);
/* channels-last [B,F,h*w,ld] (first c channels) -> [B,C,F,h,w] */
int mvoc_tokens_to_ncfhw_f16(const void* x, void* out, int32_t b, int32_t c, int32_t f, int32_t hw, int32_t ld,
                             void* stream);
/* I2VGenXLTransformerTemporalEncoder (dim 4, 2 heads x 4) fused: LN -> self-attn over frames (+res) -> FF(gelu)
 * (+res) on x [B,F,hw,4] channels-last, written into out [B,F,hw,ldo] at channel offset coff.
 * params: fp16 blob {ln_g[4], ln_b[4], wq[8][4], wk[8][4], wv[8][4], wo[4][8], bo[4], w1[16][4], b1[16], w2[4][16], b2[4]} */
int mvoc_temporal_encoder4_f16(const void* x, const void* params, void* out, int32_t b, int32_t f, int32_t hw,
                               int32_t ldo, int32_t coff, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VAE encode / decode either side of the loops (pipeline_i2vgen_xl.py:771-791 decode_latents, :860-890
 * prepare_image_latents, :893-920 encode_vae_video -> diffusers AutoencoderKL).  The convolutions, GroupNorms and the
 * mid-block attention's projections run through the entries above (mvoc_gemm_f16 incl. pad_mode = 1 for the encoder's
 * Downsample2D(padding=0), mvoc_groupnorm_f16); what they need in addition:
 *
 * Extents (enforced by tests/test_stem_contract_gpu.py; the common rules stand above, under "Stem / small ops"):
 *   conv1x1_small    reads x[rows][cin], w[cout][cin], bias[cout] (NULL: none); writes out[rows][cout]: fp32 sum + bias, rounded once.
 *                    -1: cin or cout above 64.
 *   softmax_rows     reads and writes x[rows][cols] in place and nothing else; exp and sum in fp32, one rounding (a result is the fp64
 *                    softmax rounded to fp16, or its fp16 neighbour where the fp32 error reaches across a rounding boundary).  x must be
 *                    16-byte aligned (rows move as 16-byte vectors).  -1: cols % 8 != 0, x misaligned.
 *   gaussian_sample  reads mean[n], logvar[n], noise[n], writes out[n]; a NaN logvar gives NaN (torch.clamp keeps it).
 *   scale            reads x[n], writes out[n] = fp16(fp32(float(scale) * x)).
 *   image_to_tokens  reads x[n][c][hw], writes out[n hw][c].
 *   tokens_to_image  reads x[n hw][ld] in the columns [0, c) only, writes out[n][c][hw].  -1: ld < c.
 * ------------------------------------------------------------------------------------------- */
/* 1x1 conv over a handful of channels on channels-last rows: out[r][o] = sum_c x[r][c] w[o][c] + bias[o]
 * (AutoencoderKL.quant_conv 8 -> 8, post_quant_conv 4 -> 4); cin, cout <= 64 */
int mvoc_conv1x1_small_f16(const void* x, const void* w, const void* bias, void* out, int64_t rows, int32_t cin,
                           int32_t cout, void* stream);
/* in-place softmax over the rows of a contiguous [rows][cols] fp16 matrix (fp32 math): the score matrix of the VAE's
 * single-head attention (head_dim 512; Attention(residual_connection=True) in UNetMidBlock2D), cols % 8 == 0 */
int mvoc_softmax_rows_f16(void* x, int64_t rows, int32_t cols, void* stream);
/* vae.encode(x).latent_dist.sample() (diffusers DiagonalGaussianDistribution): out = mean + exp(0.5*clamp(logvar,-30,20)) * noise,
 * each eager fp16 op rounded; and python-float * fp16 tensor (latents * scaling_factor, 1/scaling_factor * latents:
 * pipeline_i2vgen_xl.py:772, 869, 911) with the reference's fp32-then-fp16 double rounding */
int mvoc_gaussian_sample_f16(const void* mean, const void* logvar, const void* noise, void* out, int64_t n, void* stream);
int mvoc_scale_f16(const void* x, void* out, int64_t n, double scale, void* stream);
/* [n][c][hw] images / latents (reference NCHW) <-> channels-last rows [n*hw][c] (ld >= c on the way back) */
int mvoc_image_to_tokens_f16(const void* x, void* out, int32_t n, int32_t c, int32_t hw, void* stream);
int mvoc_tokens_to_image_f16(const void* x, void* out, int32_t n, int32_t c, int32_t hw, int32_t ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mask preprocessing on the device (reference i2vgen-xl/utils.py:92-154): after PNG decode + convert("L") on the
 * host, PIL's `mask.resize((W//8, H//8))` (BICUBIC, the 8-bit fixed-point path: 22 fractional bits, horizontal pass rounded to
 * uint8, then vertical) reproduced bit for bit from host-built coefficient tables (per output index {xmin, n} and n int32
 * weights, row pitch ksize), then float = v/255 in fp16 and bool = v > 10 (cv.threshold(.., 10, 255) / 255 -> bool).
 *   in [n][H][W] u8, tmp [n][H][w] u8, out [n][h][w] u8;  float_mask fp16 / bool_mask u8 of the same element count
 *
 * Extents (enforced by tests/test_stem_contract_gpu.py; the common rules stand under "Stem / small ops"):
 *   mask_resize_u8  reads in[n][H][W], bounds_h[w][2], kk_h[w][ksize_h] (of row xx its first bounds_h[xx][1] weights), bounds_v[h][2],
 *                   kk_v[h][ksize_v]; writes tmp[n][H][w] (the horizontal pass, PIL's resize to (w, H)) and out[n][h][w], both bit for
 *                   bit PIL's, the clip to 0 and 255 included.  The tables must come from mvoc_amd.utils.pil_bicubic_tables(W, w) and
 *                   (H, h): a window that leaves [0, W) or [0, H) is not checked.
 *   mask_finish     reads v[n]; writes float_mask[n] = fp16(fp32(v) / 255) and bool_mask[n] = v > 10 (1 or 0).
 * ------------------------------------------------------------------------------------------- */
int mvoc_mask_resize_u8(const void* in, void* tmp, void* out, int32_t n, int32_t H, int32_t W, int32_t h, int32_t w,
                        const int32_t* bounds_h, const int32_t* kk_h, int32_t ksize_h, const int32_t* bounds_v,
                        const int32_t* kk_v, int32_t ksize_v, void* stream);
int mvoc_mask_finish(const void* v, void* float_mask, void* bool_mask, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conditioning prep: the embedding stages of the CLIP towers the reference runs through transformers
 * (pipeline_i2vgen_xl.py:739-769 `_encode_image` -> CLIPVisionModelWithProjection, :552-737 `encode_prompt` -> CLIPTextModel);
 * the transformer stacks themselves are mvoc_gemm_f16 / mvoc_layernorm_f16 / mvoc_flash_attn_f16 (head_dim 96 | causal).
 *   clip_patches: NCHW fp16 pixels [nimg,3,size,size] -> im2col rows [nimg*(size/patch)^2, kpad] of the patch-embedding conv
 *                 (k = (c, py, px) like Conv2d's weight.view(N, -1); columns >= 3*patch^2 are zero)
 *   clip_embed  : out[row] = src(row) + pos[row % t]; src = table[ids[row]] (text: token + position embedding), or with
 *                 ids == NULL the class embedding at t == 0 and patch row (row/t)*(t-1) + (row%t) - 1 otherwise (vision)
 *
 * Extents (enforced by tests/test_stem_contract_gpu.py; the common rules stand under "Stem / small ops"):
 *   clip_patches  reads pixels[nimg][3][size][size]; writes out[nimg (size/patch)^2][kpad], every column: the columns at and past
 *                 3 patch^2 are WRITTEN as zero, not left.  -1: size % patch != 0, kpad < 3 patch^2.
 *   clip_embed    reads pos[t][c]; with ids: ids[rows] and the rows of table[.][c] they name (0 <= ids[row] < the table's rows is the
 *                 caller's promise, not checked), cls is not read; with ids == NULL: cls[c] and table[(rows / t)(t - 1)][c], which at
 *                 t == 1 is never read (the pointer must still be non-NULL).  Writes out[rows][c], the exact sum rounded once.  table,
 *                 cls, pos and out must be 16-byte aligned (rows move as 16-byte vectors).  -1: c % 8 != 0, rows % t != 0, ids and cls
 *                 both NULL, a misaligned pointer.
 * ------------------------------------------------------------------------------------------- */
int mvoc_clip_patches_f16(const void* pixels, void* out, int32_t nimg, int32_t size, int32_t patch, int32_t kpad, void* stream);
int mvoc_clip_embed_f16(const void* table, const int32_t* ids, const void* cls, const void* pos, void* out, int64_t rows,
                        int32_t t, int32_t c, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RCCL exchanges of the frame-axis shard (SURVEY 8b `allgather_frames`, 8e / BASELINE configs[3]: one long clip over the GPUs
 * of a node; the reference has no collective -- this is new work north_star asks for).  One process per GPU; rank 0 makes a
 * 128-byte id (mvoc_comm_unique_id), the host distributes it by any means, every rank calls mvoc_comm_init.  The exchanges
 * are asynchronous on `stream` and capturable; RCCL is resolved at run time (the copy PyTorch-ROCm already loaded, else
 * librccl.so.1), so the library loads without it and these entries then return -3.
 *   allgather: rank r's `bytes_per_rank` bytes land at recv + r*bytes_per_rank on every rank (temporal attention's K/V form)
 *   alltoall : send + j*bytes_per_peer goes to rank j, recv + i*bytes_per_peer came from rank i (frame shard <-> pixel shard)
 * ------------------------------------------------------------------------------------------- */
/* packing around the exchanges: out rows contiguous over (i0,i1,i2,i3) < dims4, source row = sum_k i_k * strides4[k]
 * (rows of c fp16, c % 8 == 0) -- frame shard [B,F/N,HW,C] <-> per-peer blocks <-> pixel shard [B,F,HW/N,C].
 * Extents (enforced by tests/test_stem_contract_gpu.py; the common rules stand under "Stem / small ops"): reads the rows of x that
 * the index reaches and the host arrays dims4[4], strides4[4]; writes out[dims4[0] dims4[1] dims4[2] dims4[3]][c], a copy bit for bit.
 * x and out must be 16-byte aligned (rows move as 16-byte vectors).  -1: c % 8 != 0, a dimension outside [1, 2^30), a misaligned
 * pointer.  That every source row lies inside x is the caller's promise, not checked. */
int mvoc_permute_rows_f16(const void* x, void* out, const int64_t* dims4, const int64_t* strides4, int32_t c, void* stream);
int mvoc_comm_unique_id(void* id128);
int mvoc_comm_init(const void* id128, int32_t rank, int32_t world, void** comm);
int mvoc_comm_destroy(void* comm);
int mvoc_allgather_frames(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int mvoc_alltoall_frames(void* comm, const void* send, void* recv, size_t bytes_per_peer, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-kernel-family timing with HIP events on the launch stream (bench.py roofline leg).
 * ------------------------------------------------------------------------------------------- */
enum { MVOC_FAM_GEMM = 0, MVOC_FAM_FLASH = 1, MVOC_FAM_TATTN = 2, MVOC_FAM_GN = 3, MVOC_FAM_LN = 4, MVOC_FAM_PNP = 5,
       MVOC_FAM_MISC = 6, MVOC_FAM_TFUSED = 7, MVOC_FAM_COUNT = 8 };
/* work unit per family: flops for GEMM / FLASH / TFUSED (MFMA-bound), bytes for the others (HBM-bound) */
int mvoc_prof_enable(int on);                  /* 1: bracket every launch with hipEvents (not capture-safe) */
int mvoc_prof_collect(double* ms_per_family, int64_t* launches_per_family, double* flops_or_bytes_per_family);
int mvoc_prof_reset(void);
/* enqueue a kernel that busy-waits `us` microseconds (lets the host run ahead so event brackets see no launch gaps) */
int mvoc_delay_us(int64_t us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVOC_HIP_H */
