/*
 * mmdyn_hip.h -- C ABI of libmmdyn_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * cnn-mvae / cnn-vae training and inference hot path of SAIC-MONTREAL/multimodal-dynamics.
 *
 * The reference has no native boundary: the path sits behind torch.nn modules
 * (mmdyn/pytorch/models/vae.py) and torch.nn.functional losses (mmdyn/pytorch/problems/problems.py).
 * Every entry point below replaces the stock ATen op(s) named in its comment (reference file:line),
 * and is what a maintainer would bind with ctypes from those modules.
 *
 * Conventions
 *   - all pointers are DEVICE pointers to fp32 unless stated; no allocation, no ownership transfer;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (graph-capturable);
 *   - return value: 0 = ok, MMDYN_ERR_* (<0) = argument error detected on the host before launch,
 *     >0 = hipError_t of the launch;
 *   - activations between layers are kept channels-last: a [rows][C] matrix whose row index is
 *     (sample, y, x); the reference's NCHW tensors appear only at the image input / logits output;
 *   - "groups": a batch of G*Bg samples made of G independent sub-batches (one per modality-subset
 *     pass of _evaluate_mvae, problems.py:473-546); train-mode BatchNorm statistics are per group.
 *
 * Buffer roles -- what a non-const pointer may hold when a launch starts (callers hand over torch.empty memory: the previous
 * step's activations, gradients, NaNs).  Every writable pointer is one of
 *   OUTPUT       every element of the declared extent is written, none is read first; prior contents (NaN / Inf included) never
 *                reach a result.  This is the default: a writable pointer without another word below is an output.  In particular
 *                  - C / C_act of the GEMMs: all rows x N columns (with ldc > N the columns N..ldc of a row are LEFT UNTOUCHED);
 *                  - stats [G][T][2][N] and the `partial` tables of mmdyn_colstats / mmdyn_bn_swish_bwd_reduce /
 *                    mmdyn_bn_eval_swish_bwd: all T tiles, a tile without rows as zeros (consumers sum over T);
 *                  - partial [chunks][taps][Cd][Cg] of the weight gradients: every chunk, a chunk that starts past the last row
 *                    as zeros (rows_per_chunk is rounded up to the 32-row K-step, so late chunks can be empty);
 *                  - ws [splitk][rows][N] of a split-K launch: every slice;
 *                  - the third plane of a plane tensor; the dmu / dlv rows of the experts PRESENT in a pass (mmdyn_poe_bwd; the
 *                    rows of an expert whose pointers are null in the pass are not touched, mmdyn_poe_bwd_avail writes zeros for
 *                    an absent (row, expert) pair); dlogit of a discarded pass (slot < 0): written as zeros;
 *                  - `out += beta * out` forms (mmdyn_wgrad_reduce canon, mmdyn_colsum out, mmdyn_linear_small_bwd dW / db,
 *                    dgamma / dbeta with beta_acc): with beta == 0 the destination is an OUTPUT and is not read (0 * NaN must not
 *                    survive); with beta != 0 it is an accumulator.
 *   SCRATCH      written before it is read inside the launch (or the launch pair), contents irrelevant before and after: the fp64
 *                `scratch` of the BatchNorm finalizers, the `scratch` of mmdyn_colsum, the slab workspace `ws` of a launch that
 *                is not split over K.
 *   ACCUMULATOR  read-modify-write, the CALLER initialises: the fp64 loss / KL sums and row tables (loss_sum, loss_slots,
 *                unmasked_slots, kl_sum, rows_out, ...: atomicAdd in arrival order, so equal to rounding, not bit for bit, between
 *                runs), running_mean / running_var / num_batches_tracked, optimiser parameters, moments and state, counters.
 *   STATE        tickets and arrival flags: zero when the launch starts, left zero.
 *   LEFT UNTOUCHED  elements outside the block a launch addresses: the columns cols_out..ld_out of mmdyn_repack2d_ld (inside the
 *                block the padding rows_in..rows_out / cols_in..cols_out IS written, as zeros), rows of another group behind an
 *                offset pointer, canon has exactly Cd * cg_canon * taps elements (the gathered columns cg_canon..Cg are dropped, not
 *                written anywhere).
 * tests/test_dirty_memory_gpu.py holds the kernels to this: the same launch on zero-, NaN- and junk-filled destinations gives the
 * same bits.
 */
#ifndef MMDYN_HIP_H
#define MMDYN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDYN_OK 0
#define MMDYN_ERR_SHAPE (-1)   /* dimension not supported by the kernel (see each function) */
#define MMDYN_ERR_NULL (-2)    /* required pointer is null */
#define MMDYN_ERR_RANGE (-3)   /* tensor too large for 32-bit element offsets */

#define MMDYN_ACT_NONE 0
#define MMDYN_ACT_SWISH 1      /* x * sigmoid(x), vae.py:331-334 */
#define MMDYN_ACT_RELU 2

/* implicit-GEMM modes (k = 4 everywhere, as in vae.py:198-206, 268-277) */
#define MMDYN_DENSE 0          /* plain rows x Cin matrix (nn.Linear, and the col-matrix GEMMs) */
#define MMDYN_CONV 1           /* gather form: out(r,c) <- in(r*s+o+kh, c*s+o+kw), 16 taps */
#define MMDYN_TCONV_S2P1 2     /* transposed k4 s2 p1, four output-parity classes of 4 taps each */
#define MMDYN_IM2COL3 3        /* k4 s2 p1 window of an NCHW 3-channel tensor gathered on the fly: virtual Cin = 64
                                  (k = ci*16 + kh*4 + kw, 48 real + 16 zero); rows = output pixels.  Lowers
                                  nn.Conv2d(3,32,4,2,1) (vae.py:198) and the backward of nn.ConvTranspose2d(32,3,4,2,1)
                                  (vae.py:277) onto the MFMA GEMMs without materialising an im2col matrix */

#define MMDYN_TCONV_S1P0 4      /* transposed k4 s1 p0 (Ho = Hi+3): rows ordered (output pixel, sample) inside a group so
                                  every tile covers one output pixel and only its 1..16 valid taps are multiplied --
                                  exactly the useful MACs, no zero padding, no column matrix.  Served for the 5x5 -> 8x8
                                  layer only (vae.py:268): the blocks walk the four-pixel quads of an 8x8 output, so any
                                  other extent -- Hi != Wi included -- is MMDYN_ERR_SHAPE.  C itself is plain NHWC */
/* Hi != Wi: the other modes take non-square extents (tests/test_exact_gpu.py holds them to exact results).  The kernels
 * specialised to the model's square layers -- the patch-resident k4 s2 p1 kernel (N = 32), its plane form and the 3-channel
 * first / last-layer kernels -- decline such a shape and the launch runs on the generic kernels; mmdyn_igemm_planes_served answers
 * 0 for a non-square shape only they would serve. */

const char* mmdyn_version(void);
/* ABI revision of this header.  It changes whenever an exported signature or a workspace requirement changes (round 4 added
 * the `ws` argument of mmdyn_igemm_nt_dgrad_act / _dgrad_bn and the slab workspace of large launches: revision 4; round 5 the
 * plane-packed weight kinds of the pack plan: revision 5; round 6 the `zdst` field of mmdyn_pass_experts, the separate, nullable
 * `arrival_flags` argument of mmdyn_igemm_nt_mx / _dgrad_bn / _dgrad_act (MMDYN_IGEMM_FLAG_WORDS zeroed words of its own; the layout
 * and size of `ws`, mmdyn_igemm_slab_floats*, did not change) and new entry points: revision 6; the per-sample
 * ELBO entry points (mmdyn_*_rows*) and the importance-weighted bound (mmdyn_iw_*) were added without touching an existing signature or
 * workspace and keep revision 6).  A binding checks mmdyn_abi_version() == MMDYN_ABI_VERSION right after
 * loading the library (mmdyn_hip/_lib.py does) so that a caller built against an older header fails at load time instead of
 * passing its stream handle where the library now expects a workspace pointer. */
#define MMDYN_ABI_VERSION 6
int mmdyn_abi_version(void);

/* ---- MFMA implicit GEMM, "NT" form ---------------------------------------------------------
 * C[row][n] = act( sum_{tap,ci} A_tap[row][ci] * Bp[widx(tap)][n][ci] + bias[n] )
 * Replaces: nn.Conv2d forward (vae.py:200,203,206), nn.ConvTranspose2d forward (vae.py:271,274),
 * their input-gradient kernels, and nn.Linear forward / input-gradient (vae.py:211,215,216,264).
 *   A      : NHWC activations [G*Bg][Hi][Wi][Cin]
 *   Bp     : packed weights [taps][N][Cin] (see mmdyn_pack_conv_weight)
 *   C      : NHWC output [G*Bg][Ho][Wo] rows of stride ldc (>= N); pre-activation (+bias)
 *   C_act  : optional second output = act(C) (null: none)
 *   stats  : optional per-tile BatchNorm partial sums [G][T][2][N], T = mmdyn_igemm_stat_tiles(...)
 *   splitk : >1 only for DENSE: partial products go to `ws` ([splitk][rows][N]) and
 *            mmdyn_splitk_reduce finishes (bias/act/second output are applied there).
 *   ws     : with splitk == 1 the LARGE launches (persistent stream-K kernel, csrc/igemm_wsp.hip) park the pieces of tiles
 *            that straddle two blocks there: ws must hold mmdyn_igemm_slab_floats(...) floats whenever that query answers
 *            > 0 (MMDYN_ERR_NULL otherwise); NULL is fine when it answers 0.  Same rule for mmdyn_igemm_nt_mx
 *            (mmdyn_igemm_slab_floats_mx).
 *   arrival_flags (mmdyn_igemm_nt_mx, _dgrad_bn, _dgrad_act; revision 6): MMDYN_IGEMM_FLAG_WORDS uint32 words that are ZERO when the
 *            launch starts and that the launch leaves zero, owned by this launch until it has completed (a launch captured
 *            into a graph owns them for the graph's life).  With them the LAB build of the library (make lab) finishes a tile
 *            whose K range straddles several blocks INSIDE the launch -- the piece that arrives last on the tile's word sums the
 *            pieces in K order and runs the epilogue: same results bit for bit, no fix-up launch.  The PRODUCT library accepts
 *            and ignores the argument: that form measured 3-6 % slower on the train step (docs/LAB_NOTES.md H.a), so slabs + the
 *            fix-up launch stay.  NULL: slabs + the fix-up launch in either build.
 * Requirements: Cin % 32 == 0, N % 32 == 0.  v_mfma_f32_32x32x2_f32, fp32 in / fp32 accumulate. */
#define MMDYN_IGEMM_FLAG_WORDS 8192
/* Buffers: C / C_act and stats are OUTPUTS (every row x N column; every one of the T tiles, a tile without rows as zeros); ws is an
 * OUTPUT with splitk > 1 (every slice) and SCRATCH otherwise; none of them is read before it is written. */
int mmdyn_igemm_nt(const float* A, const float* Bp, const float* bias, float* C, float* C_act,
                   float* stats, float* ws, int mode, int G, int Bg, int Hi, int Wi, int Cin,
                   int Ho, int Wo, int N, int ldc, int stride, int offset, int act, int splitk,
                   void* stream);
/* Input-gradient GEMM with the backward of a plain activation in its epilogue (replaces the separate element-wise
 * x * act'(u) pass of loss.backward() through Swish / ReLU, vae.py:14-19, 215, 267, 331-334):
 *     C = (A x Bp) * act'(u),   u = the layer's saved pre-activation at the C positions (row stride N),
 * act = MMDYN_ACT_SWISH or MMDYN_ACT_RELU (for ReLU u may be the activated output: same sign).  No bias, second output,
 * statistics or split-K.  flags: 0 = fp32 everywhere; otherwise as mmdyn_igemm_nt_mx (bit 3: u is bf16).
 * ws: workspace of mmdyn_igemm_slab_floats(...) floats (NULL when that is 0). */
int mmdyn_igemm_nt_dgrad_act(const void* A, const void* Bp, void* C, const void* u, int act, int mode, int G, int Bg,
                             int Hi, int Wi, int Cin, int Ho, int Wo, int N, int stride, int offset, int flags,
                             float* ws, uint32_t* arrival_flags, void* stream);
/* Input-gradient GEMM with the BatchNorm+Swish backward of the PRECEDING layer fused into its epilogue.
 * The tile of dL/d(activation) never reaches HBM as such: with y the layer's saved pre-BatchNorm output (same
 * rows/columns as C) and xhat = (y - mean[g]) * rstd[g], the kernel writes
 *     C = du = dL/da * swish'(gamma*xhat + beta)
 * and the per-tile column sums (du, du*xhat) into stats[G][T][2][N] (T = mmdyn_igemm_stat_tiles), which feed
 * mmdyn_bn_bwd_finalize directly -- the separate reduction pass (mmdyn_bn_swish_bwd_reduce: one more read of da
 * and y) disappears; mmdyn_bn_swish_bwd_apply(da_is_du = 1) finishes the layer.  bf16: 0 = fp32 matrix cores,
 * 1 = bf16, 2 = fp16 operands (T = mmdyn_igemm_stat_tiles_bf16 for both), 3 = fp32 arithmetic with the three-term split allowed
 * (flag bit 7 of mmdyn_igemm_nt_mx; T = mmdyn_igemm_stat_tiles_mx(..., 128)).  No bias / activation / split-K here.
 * ws: workspace of mmdyn_igemm_slab_floats(...) floats (NULL when that is 0). */
int mmdyn_igemm_nt_dgrad_bn(const float* A, const float* Bp, float* C, float* stats, const float* y,
                            const float* mean, const float* rstd, const float* gamma, const float* beta,
                            int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N,
                            int stride, int offset, int bf16, float* ws, uint32_t* arrival_flags, void* stream);
/* Workspace (floats) the fp32 launch of a shape wants in its `ws` argument when it is not split over K: the persistent,
 * stream-K-scheduled ring kernel (csrc/igemm_wsp.hip) accumulates a tile whose K range straddles two blocks in pieces and
 * parks the pieces there for its fix-up launch.  0 = none (ws may be NULL). */
int mmdyn_igemm_slab_floats(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N);

/* Same contract, bf16 matrix cores: the fp32 operands are rounded to bf16 (round-to-nearest-even) on their way
 * into the MFMA (v_mfma_f32_32x32x16_bf16), products are accumulated in fp32, everything in HBM stays fp32.
 * The reduced-precision mode of BASELINE configs[2] ("bf16"); never used by the fp32 path. */
int mmdyn_igemm_nt_bf16(const float* A, const float* Bp, const float* bias, float* C, float* C_act,
                        float* stats, float* ws, int mode, int G, int Bg, int Hi, int Wi, int Cin,
                        int Ho, int Wo, int N, int ldc, int stride, int offset, int act, int splitk,
                        void* stream);
/* Same contract, fp16 matrix cores: operands rounded to IEEE half (RNE) on their way into v_mfma_f32_32x32x16_f16, fp32
 * accumulate, everything in HBM fp32 -- "MFMA fp16 conv with fp32 accumulate" of BASELINE configs[4].  Partial-sum tile
 * count: mmdyn_igemm_stat_tiles_bf16. */
int mmdyn_igemm_nt_f16(const float* A, const float* Bp, const float* bias, float* C, float* C_act,
                       float* stats, float* ws, int mode, int G, int Bg, int Hi, int Wi, int Cin,
                       int Ho, int Wo, int N, int ldc, int stride, int offset, int act, int splitk,
                       void* stream);
/* T of the `stats` argument for the shape: what mmdyn_igemm_nt / mmdyn_igemm_nt_dgrad_bn(bf16 = 0) write ... */
int mmdyn_igemm_stat_tiles(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N);
/* ... and what the bf16 matrix-core variants (mmdyn_igemm_nt_bf16, mmdyn_igemm_nt_mx, dgrad_bn(bf16 = 1)) write */
int mmdyn_igemm_stat_tiles_bf16(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N);
/* ... and of the mixed-storage entry point mmdyn_igemm_nt_mx for the given flags (launches whose two operands are both 16-bit
 * in HBM may run the persistent ring kernel, csrc/igemm_wsp.hip, which writes one partial tile per wave row); flags == 0:
 * mmdyn_igemm_stat_tiles.  mmdyn_igemm_slab_floats_mx: the `ws` workspace of such a launch (see mmdyn_igemm_slab_floats). */
int mmdyn_igemm_stat_tiles_mx(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N, int flags);
int mmdyn_igemm_slab_floats_mx(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N, int flags);
/* Grouped dense GEMM (round 4): G independent problems of ONE shape in one launch,
 *   C_g[rows][N] = A_g[rows][K] . Bp_g[N][K]^T (+ bias_g),   g = 0 .. G-1,
 * group g at A + g*rows*K, Bp + g*N*K, bias + g*N, C / C_act / u + g*rows*N.  Replaces the three nn.Linear pairs
 * linear_means | linear_log_var (vae.py:211-216, 239-240) of the visual, tactile and pose encoders at the product-of-experts
 * join, forward and input gradient: 1024 x 512 x 512 each, half a chip's worth of tiles when launched alone.
 * u != NULL: C = (A . Bp^T) * act'(u) (activation backward in the epilogue; bias and C_act must be NULL).
 * flags: as mmdyn_igemm_nt_mx (0 = fp32 everywhere).  K % 32 == 0, N % 32 == 0. */
int mmdyn_igemm_nt_grouped(const void* A, const void* Bp, const float* bias, void* C, void* C_act, const void* u, int G,
                           int rows, int K, int N, int act, int flags, void* stream);
/* C / C_act: OUTPUTS (ws is read only). */
int mmdyn_splitk_reduce(const float* ws, const float* bias, float* C, float* C_act, int splitk,
                        int rows, int N, int act, void* stream);

/* ---- MFMA weight gradient, "TN" form -------------------------------------------------------
 * partial[chunk][tap][cd][cg] = sum_{rows in chunk} D[row][cd] * G_tap[row][cg]
 * Replaces the weight-gradient kernels of Conv2d / ConvTranspose2d / Linear.
 *   D  : dense rows [Bt*Hr*Wr][Cd];  Gt : gathered operand, NHWC [Bt][Hi][Wi][Cg]
 *   mode DENSE: one tap, Gt rows == D rows.  mode CONV: 16 taps, pixel (r*s+o+kh, c*s+o+kw).
 * mmdyn_wgrad_reduce sums the chunks and writes the reference's canonical layout:
 *   perm 0: canon[cd][cg][tap] (conv [Cout][Cin][4][4] / convT [Cin][Cout][4][4]; Linear [out][in])
 *   perm 1: linear with permuted columns, cg = hw*256+c -> canon[cd][c*25+hw]  (Encoder fc_net.0)
 *   perm 2: linear with permuted rows,    cd = hw*256+c -> canon[c*25+hw][cg]  (Decoder upsample.0)
 *   cg_canon <= Cg drops zero-padded gathered columns (the 48 -> 64 padded first/last layers).
 * Requirements: Cd % 32 == 0, Cg % 32 == 0. */
/* partial: OUTPUT, every chunk -- a chunk that starts past the last row (rows_per_chunk is rounded up to the 32-row K-step) is
 * written as zeros, so the caller need not clear it.  Same for the _bf16 / _f16 / _mx / _grouped / mmdyn_wgrad_out3_bn forms. */
int mmdyn_wgrad_tn(const float* D, const float* Gt, float* partial, int mode, int Bt, int Hr, int Wr,
                   int Cd, int Hi, int Wi, int Cg, int stride, int offset, int chunks, void* stream);
/* bf16 matrix cores (v_mfma_f32_32x32x8_bf16), fp32 accumulate; see mmdyn_igemm_nt_bf16 */
int mmdyn_wgrad_tn_bf16(const float* D, const float* Gt, float* partial, int mode, int Bt, int Hr, int Wr,
                        int Cd, int Hi, int Wi, int Cg, int stride, int offset, int chunks, void* stream);
/* fp16 matrix cores (v_mfma_f32_32x32x8_f16), fp32 accumulate; see mmdyn_igemm_nt_f16 */
int mmdyn_wgrad_tn_f16(const float* D, const float* Gt, float* partial, int mode, int Bt, int Hr, int Wr,
                       int Cd, int Hi, int Wi, int Cg, int stride, int offset, int chunks, void* stream);
/* recommended `chunks` (a multiple of 4) for mmdyn_wgrad_tn; partial must hold chunks*taps*Cd*Cg floats */
/* Grouped weight gradient (round 4; DENSE): group g owns rows [g*rows, (g+1)*rows) of D [G*rows][Cd] and Gt [G*rows][Cg];
 * partial is [chunks][G][Cd][Cg], so ONE mmdyn_wgrad_reduce(partial, canon, chunks, 1, G*Cd, Cg, Cg, 0, beta) writes the G
 * gradients [G][Cd][Cg] (the fused engine keeps the heads' weights of the three encoders adjacent).  chunks as
 * mmdyn_wgrad_chunks_mx(DENSE, rows, Cd, Cg, flags); flags as mmdyn_wgrad_tn_mx (not both operands 16-bit). */
int mmdyn_wgrad_tn_grouped(const void* D, const void* Gt, float* partial, int G, int rows, int Cd, int Cg, int chunks,
                           int flags, void* stream);
/* Round 4, SURVEY.md section 7 step 5 (BatchNorm-apply + Swish fused into the neighbouring kernels): the weight gradient of
 * the decoder's last layer nn.ConvTranspose2d(32, 3, 4, 2, 1) (vae.py:277) with the BatchNorm2d + Swish in front of it
 * (vae.py:275-276) recomputed on the operand fetch.  y [G*Bg][Hr][Hr][32]: the pre-BatchNorm tensor (fp32; y_b16 = 1 bf16,
 * 2 IEEE half); mean / rstd [G][32]; Gt: the NCHW logit gradient [G*Bg][3][2Hr][2Hr]; partial [chunks][32][64] as
 * mmdyn_wgrad_tn(MMDYN_IM2COL3) writes it (chunks = mmdyn_wgrad_chunks(MMDYN_IM2COL3, ...); any chunks >= 1 is taken, slab c holds
 * the c-th range of ceil(units / chunks) units, a unit being a 32-pixel segment of a row of y).  Square images of Hr = 32, 64 or 128
 * only: there is one extent argument, and every other Hr is MMDYN_ERR_SHAPE before anything is launched. */
int mmdyn_wgrad_out3_bn(const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* Gt, float* partial, int G, int Bg, int Hr, int chunks, int y_b16, void* stream);
int mmdyn_wgrad_chunks(int mode, int rows, int Cd, int Cg);
/* ... for the kernel the flags of mmdyn_wgrad_tn_mx select (both operands 16-bit in HBM: the all-16-bit kernels' tiles; bit 7
 * alone: the three-term-split kernels, whose LDS planes let fewer blocks share a CU) */
int mmdyn_wgrad_chunks_mx(int mode, int rows, int Cd, int Cg, int flags);
/* canon has exactly Cd * cg_canon * taps elements: OUTPUT with beta == 0 (not read: a stale NaN must not survive 0 * NaN),
 * ACCUMULATOR with beta != 0.  The gathered columns cg_canon..Cg are dropped, written nowhere. */
int mmdyn_wgrad_reduce(const float* partial, float* canon, int chunks, int taps, int Cd, int Cg,
                       int cg_canon, int perm, float beta, void* stream);
/* The dense weight gradient written ONCE: mmdyn_wgrad_tn_grouped + mmdyn_wgrad_reduce(taps = 1, Cd' = G*Cd) in one launch without
 * the slabs -- one block per (channel tile, group) sums its `chunks` row pieces itself, in the slab reduction's order, so canon
 * [G*Cd][cg_canon] holds the same bits as after the two launches.  chunks as mmdyn_wgrad_chunks_mx(DENSE, rows, Cd, Cg, flags);
 * perm / cg_canon / beta as mmdyn_wgrad_reduce (perm 1 / 2: G = 1; perm 1: cg_canon = Cg).  Serves what mmdyn_wgrad_canon_served accepts, else
 * MMDYN_ERR_SHAPE (added without touching an existing signature: revision 6). */
int mmdyn_wgrad_tn_canon(const void* D, const void* Gt, float* canon, int G, int rows, int Cd, int Cg, int cg_canon, int perm,
                         float beta, int chunks, int flags, void* stream);
/* Host only: 1 when mmdyn_wgrad_tn_canon serves (rows, Cd, Cg, groups) under `flags`, 0 otherwise -- plane operands, 16-bit
 * storage, channel tiles whose waves split the rows, more than 64 chunks or fewer than 65536 elements (the slab reduction sums
 * those in another order). */
int mmdyn_wgrad_canon_served(int rows, int Cd, int Cg, int groups, int flags);

/* ---- weight packing (canonical reference layout -> GEMM operand layout) --------------------- */
/* Wc[d0][d1][16] -> P[tap][d0][d1] (swap=0) or P[tap][d1][d0] (swap=1) */
int mmdyn_pack_conv_weight(const float* Wc, float* P, int d0, int d1, int swap, void* stream);
/* generic 2-D repack: out[r][c] (rows_out x cols_out, zero padded) = in[...] with
 * mode 0: copy/pad in[r][c] (in is rows_in x cols_in)
 * mode 1: transpose  out[r][c] = in[c][r]
 * mode 2: column permute out[r][hw*256+ch] = in[r][ch*25+hw]
 * mode 3: row permute    out[hw*256+ch][c] = in[ch*25+hw][c]
 * mode 4: transpose of mode 2: out[hw*256+ch][c] = in[c][ch*25+hw]
 * mode 5: transpose of mode 3: out[r][hw*256+ch] = in[ch*25+hw][r] */
int mmdyn_repack2d(const float* in, float* out, int rows_in, int cols_in, int rows_out, int cols_out,
                   int mode, void* stream);

/* mmdyn_repack2d writing a rows_out x cols_out block into a wider matrix (row stride ld_out >= cols_out) */
/* Inside the block the padding rows_in..rows_out / cols_in..cols_out is written (zeros); the columns cols_out..ld_out of each row are
 * LEFT UNTOUCHED. */
int mmdyn_repack2d_ld(const float* in, float* out, int rows_in, int cols_in, int rows_out, int cols_out,
                      int ld_out, int mode, void* stream);
/* the same two packs with a 16-bit destination (RNE; half = 0: bf16, half = 1: IEEE half): in the 16-bit storage modes
 * the weights are packed straight to the matrix cores' operand type, which halves the weight bytes every implicit-GEMM
 * block pulls through L2 */
int mmdyn_pack_conv_weight_b16(const float* Wc, void* P, int d0, int d1, int swap, int half, void* stream);
int mmdyn_repack2d_ld_b16(const float* in, void* out, int rows_in, int cols_in, int rows_out, int cols_out,
                          int ld_out, int mode, int half, void* stream);
/* A whole step's weight repacks in one launch.  `plan_dev` is a DEVICE array of n entries (built once: the
 * parameter storage of a training run does not move).  kind 0..5 = mmdyn_repack2d modes with an output leading
 * dimension ld_out (>= cols_out); kind 100 / 101 = mmdyn_pack_conv_weight with swap 0 / 1 (rows_in = d0,
 * cols_in = d1). */
typedef struct {
  const float* src;
  float* dst;
  int kind, rows_in, cols_in, rows_out, cols_out, ld_out;
  int dst_bf16;   /* 1: dst is a bf16 tensor (ld_out in elements), 2: an IEEE-half tensor; the GEMM operands of the 16-bit modes;
                     3 (kinds 100 / 101 only): dst is a PLANE tensor, rows (tap, x) of [plane][y] bf16 -- the exact three-term split
                     of the packed weight (mmdyn_split_planes of the kind's fp32 output), the Bp of the plane launches */
} mmdyn_pack_entry;
int mmdyn_pack_plan(const mmdyn_pack_entry* plan_dev, int n, void* stream);

/* ---- first / last layer helpers (3-channel NCHW side) --------------------------------------- */
/* col[(b*Ho+ho)*Wo+wo][ci*16+kh*4+kw] = x[b][ci][2ho-1+kh][2wo-1+kw], columns 48..63 zero.
 * x: NCHW [Bt][3][H][W]; col: [Bt*(H/2)*(W/2)][64].  Lowers nn.Conv2d(3,32,4,2,1) (vae.py:198) and the
 * backward of nn.ConvTranspose2d(32,3,4,2,1) (vae.py:277) onto the MFMA GEMMs above. */
int mmdyn_im2col_nchw3(const float* x, float* col, int Bt, int H, int W, void* stream);
/* transposed-conv scatter as a gather: out(ho,wo,c) = sum_{kh,kw} col[(hi,wi)][...], hi=(ho+p-kh)/s.
 *   tap_major=1: col column = tap*C + c (NHWC out, [Bt][Ho][Wo][C]);
 *   tap_major=0: col column = c*16 + tap and the output is NCHW [Bt][C][Ho][Wo] (logits). */
int mmdyn_col2im_k4(const float* col, float* out, int Bt, int Hi, int Wi, int Ho, int Wo, int C,
                    int ldcol, int stride, int pad, int tap_major, void* stream);

/* nn.ConvTranspose2d(32, 3, 4, 2, 1) forward (vae.py:277) as a direct LDS-tiled VALU kernel: a is NHWC
 * [Bt][Hi][Wi][32], w the reference's [32][3][4][4], out NCHW logits [Bt][3][2Hi][2Wi]; Hi, Wi % 16 == 0. */
int mmdyn_tconv_out3_fwd(const float* a, const float* w, float* out, int Bt, int Hi, int Wi, void* stream);
/* ... fused with the BatchNorm2d + Swish in front of it (vae.py:275-277): y [G*Bg][Hi][Wi][32] is the pre-BatchNorm output of the
 * layer below (fp32; b16 = 1 bf16, 2 IEEE half), mean / rstd [G][32] its batch statistics; the activation is applied while
 * the input tile is staged, the activated tensor never exists in HBM.  Like mmdyn_tconv_out3_fwd this form and the three loss forms
 * below take any Hi, Wi that are multiples of 16, Hi != Wi included (anything else: MMDYN_ERR_SHAPE); the padding around the image is
 * zero AFTER the activation. */
int mmdyn_tconv_out3_bn_fwd(const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            const float* w, float* out, int G, int Bg, int Hi, int Wi, int b16, void* stream);
/* ... and with the reconstruction term of the ELBO in its epilogue (round 6): F.binary_cross_entropy_with_logits(recon, target,
 * reduction='sum') of problems.py:433-437 (with `mask`, [Bg][mask_channels][2Hi][2Wi], mask_channels 1 or 3: torch.mul of logits and
 * target with the loss mask first, problems.py:445-447; `unmasked_slots`, may be null, then also gets the plain sums) for the G
 * groups of the batch against ONE target [Bg][3][2Hi][2Wi]: loss_slots[slot_of_group[g]] += sum over group g (slot < 0: a discarded
 * pass -- zero gradient, no loss); dlogit [G*Bg][3][2Hi][2Wi] (null in evaluation) = (sigmoid(logit) - target) * grad_scale, the
 * gradient the backward of the layer consumes.  The logits themselves are written only for group `logits_group` (`logits`
 * [Bg][3][2Hi][2Wi]; -1: for all groups, [G*Bg]...; `logits` null: for none) -- the reconstruction the caller publishes
 * (problems.py:537-545).  Element arithmetic identical to mmdyn_bce_logits_groups. */
int mmdyn_tconv_out3_bn_bce(const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            const float* w, float* logits, int logits_group, const float* target, const float* mask,
                            int mask_channels, float* dlogit, double* loss_slots, double* unmasked_slots,
                            const int* slot_of_group, float grad_scale, int G, int Bg, int Hi, int Wi, int b16, void* stream);
/* The evaluation form of that launch with one sum per SAMPLE (the reduce=False branch, problems.py:451-456: torch.sum(e, (1, 2, 3))):
 * loss_rows[slot_of_group[g]][b] += the sum over sample b of group g, loss_rows / unmasked_rows [n_slots][Bg] double (a slot at or
 * above n_slots is MMDYN_ERR_SHAPE).  Same arguments otherwise, no gradient output; the same kernel (a block of its grid never spans
 * two samples), so the logits of the passes nobody reads are not written here either. */
int mmdyn_tconv_out3_bn_bce_rows(const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 const float* w, float* logits, int logits_group, const float* target, const float* mask,
                                 int mask_channels, double* loss_rows, double* unmasked_rows, const int* slot_of_group,
                                 int n_slots, int G, int Bg, int Hi, int Wi, int b16, void* stream);

/* ---- train-mode BatchNorm2d + Swish, channels-last, per group (vae.py:201-208, 269-276) ----- */
/* column sums of y and y*y over row chunks -> partial[G][T][2][C], T = mmdyn_colstats_tiles(rows_per_group) */
/* partial: OUTPUT, all T tiles (also for mmdyn_bn_swish_bwd_reduce and the partial of mmdyn_bn_eval_swish_bwd). */
int mmdyn_colstats(const float* y, float* partial, int G, int rows_per_group, int C, void* stream);
int mmdyn_colstats_tiles(int rows_per_group);
/* partial -> mean/rstd [G][C]; running stats EMA (momentum 0.1, unbiased var) applied for the groups in
 * order, `repeat` times each (the reference re-runs identical encoder trunks: SURVEY.md 3.2);
 * num_batches_tracked (int64) += G*repeat.  running_* may be null. */
/* mean / rstd: OUTPUTS; scratch: SCRATCH (written before it is read); running_* / num_batches_tracked: ACCUMULATORS; ticket: STATE. */
int mmdyn_bn_finalize(const float* partial, float* mean, float* rstd, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, double* scratch /* [32][G][2][C] */,
                      int G, int T, int C, int rows_per_group, float eps, float momentum, int repeat,
                      uint32_t* ticket, void* stream);
/* `ticket` (here, in mmdyn_bn_bwd_finalize and in mmdyn_colsum; nullable): a zero-initialised 32-bit word in device
 * memory that no other launch in flight uses.  With it the two stages run as ONE launch: every block publishes its
 * partial sums (agent-scope release), draws a ticket, and the block that arrives last (agent-scope acquire) adds the
 * partials in the same fixed order as the separate second kernel -- bit-identical results -- and puts the word back to
 * zero (a HIP-graph replay finds it zero again).  Without it: two launches.  The two BatchNorm finalize entry points take the
 * single launch only for T < 640 (where both forms add the tile sums in the same four slices or fewer); a larger table runs as two
 * launches with or without a ticket, and the word is not touched. */
/* a = swish(gamma*(y-mean)*rstd + beta) */
int mmdyn_bn_swish_fwd(const float* y, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, float* a, int G, int rows_per_group, int C, void* stream);
/* backward, two launches: reduce -> sums[G][2][C] (+ dgamma/dbeta accumulated), then apply -> dy */
int mmdyn_bn_swish_bwd_reduce(const float* da, const float* y, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, float* partial, int G,
                              int rows_per_group, int C, void* stream);
/* sums: OUTPUT; dgamma / dbeta: OUTPUTS with beta_acc == 0 (not read), ACCUMULATORS otherwise; scratch: SCRATCH. */
int mmdyn_bn_bwd_finalize(const float* partial, float* sums, float* dgamma, float* dbeta,
                          double* scratch /* [32][G][2][C] */, int G, int T, int C, float beta_acc,
                          uint32_t* ticket, void* stream);
/* eval mode (model.eval(): nn.BatchNorm2d with training=False): mean[g][c] = running_mean[c],
 * rstd[g][c] = 1/sqrt(running_var[c] + eps), formed in fp64 and rounded once; mmdyn_bn_swish_fwd then applies them.  No buffer
 * update. */
int mmdyn_bn_eval_stats(const float* running_mean, const float* running_var, float* mean, float* rstd, int G, int C,
                        float eps, void* stream);
/* Synchronised BatchNorm across data-parallel ranks (optional): the per-channel sums are
 * collapsed to double [G][2][C], all-reduced by the host (RCCL), and the statistics / backward coefficients are
 * finished from the GLOBAL sums.  reduce_partials: scratch like mmdyn_bn_finalize.  finalize_sums: n = global rows per
 * group.  bwd_finalize_sums: dgamma/dbeta (nullable) = local parameter gradients (the gradient all-reduce adds the
 * ranks); sums_f (nullable) = float copy of the sums times sums_scale (global sums x n_local/n_global, so that
 * mmdyn_bn_swish_bwd_apply, which divides by the local row count, applies the global means). */
int mmdyn_bn_reduce_partials(const float* partial, double* sums, double* scratch, int G, int T, int C, void* stream);
int mmdyn_bn_finalize_sums(const double* sums, float* mean, float* rstd, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, int G, int C, int n, float eps, float momentum, int repeat,
                           void* stream);
int mmdyn_bn_bwd_finalize_sums(const double* sums, float* sums_f, float* dgamma, float* dbeta, int G, int C,
                               float sums_scale, float beta_acc, void* stream);
/* da_is_du != 0: `da` already holds du = da * swish'(gamma*xhat+beta) (written by mmdyn_igemm_nt_dgrad_bn) */
int mmdyn_bn_swish_bwd_apply(const float* da, const float* y, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const float* sums, float* dy, int G,
                             int rows_per_group, int C, int da_is_du, void* stream);

/* ---- element-wise ---------------------------------------------------------------------------- */
int mmdyn_act_fwd(const float* u, float* h, int64_t n, int act, void* stream);
/* du = dh * act'(u) */
int mmdyn_act_bwd(const float* dh, const float* u, float* du, int64_t n, int act, void* stream);
/* nn.Dropout(p) with injected keep-masks (vae.py:213): out[p][b][:] = h[b][:] * mask[p][b][:] / (1-p_drop)
 * for P passes sharing one trunk output h[B][H];  backward sums the P masked gradients. */
int mmdyn_dropout_expand(const float* h, const uint8_t* masks, float* out, int P, int B, int H,
                         float p_drop, void* stream);
int mmdyn_dropout_reduce(const float* dout, const uint8_t* masks, float* dh, int P, int B, int H,
                         float p_drop, const float* u /* nullable [B][H]: dh *= act'(u), the activation in front of the
                         dropout (vae.py:213-216) */, int act, void* dh_planes /* nullable (revision 6): dh also as a plane tensor,
                         rows of [plane][H] bf16 -- the operand of a plane launch */, void* stream);
/* keep-masks / N(0,1) draws from a counter-based Philox-4x32-10 stream (throughput runs; parity runs inject
 * tensors).  The stream position is offset + *offset_dev (offset_dev may be null): keeping the running position
 * in device memory and bumping it with mmdyn_counter_add makes a captured HIP graph draw fresh numbers on replay. */
int mmdyn_random_masks(uint8_t* masks, int64_t n, float p_drop, uint64_t seed, uint64_t offset,
                       const uint64_t* offset_dev, void* stream);
int mmdyn_random_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                        void* stream);
int mmdyn_counter_add(uint64_t* counter, uint64_t inc, void* stream);
/* out[c] (+)= sum_r x[r][c]   (bias gradients); deterministic two-stage sum, scratch holds
 * mmdyn_colsum_chunks(rows) * C floats; perm 2 = the upsample-bias permutation hw*256+c -> c*25+hw; C % 4 == 0 */
/* out: OUTPUT with beta == 0 (not read), ACCUMULATOR otherwise; scratch: SCRATCH. */
int mmdyn_colsum(const float* x, float* out, float* scratch, int rows, int C, int perm, float beta, uint32_t* ticket,
                 void* stream);
int mmdyn_colsum_chunks(int rows);
/* out = x * s[0], s in device memory (chain rule through a scalar loss term without a host sync) */
int mmdyn_scale_dev(const float* x, const float* s, float* out, int64_t n, void* stream);
/* Gradient buckets on the wire in bf16 (data parallel, 16-bit storage modes; the reference has no
 * counterpart: problems.py:52, 388 train on one device): round the fp32 bucket to bf16 (RNE) in front of the all-reduce,
 * widen it back behind it.  src / dst 16-byte (fp32 side) and 8-byte (bf16 side) aligned. */
int mmdyn_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int mmdyn_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* n <= MMDYN_COPY_MANY_MAX device-to-device copies (src[i] -> dst[i], bytes[i] bytes; host arrays of device pointers) as ONE
 * launch: a batch (inputs + targets of problems.py:148-156) moved into the static buffers of a captured step.  Segments must not
 * overlap.  (The reference hands its batch to the model by reference; there is no counterpart call.) */
#define MMDYN_COPY_MANY_MAX 8
int mmdyn_copy_many(const void* const* src, void* const* dst, const int64_t* bytes, int n, void* stream);
/* sum of P row blocks: out[b][:] = sum_p x[p][b][:] */
int mmdyn_sum_blocks(const float* x, float* out, int P, int64_t n, void* stream);
/* tiny Linear layers of the 7-DoF pose MLP (K or N == 7; vae.py:117-123): y = x W^T + b */
int mmdyn_linear_small_fwd(const float* x, const float* W, const float* b, float* y, int rows, int K,
                           int N, int act, void* stream);
/* dx: OUTPUT; dW / db: OUTPUTS with beta == 0 (not read), ACCUMULATORS otherwise. */
int mmdyn_linear_small_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW,
                           float* db, int rows, int K, int N, float beta, void* stream);

/* ---- product of experts + reparametrisation + KL (vae.py:311-318, 52-61; problems.py:429) --- */
#define MMDYN_MAX_PASSES 8
#define MMDYN_MAX_EXPERTS 4
typedef struct {
  const float* mu[MMDYN_MAX_EXPERTS];   /* expert means (visual, tactile, pose, spare); null = absent */
  const float* lv[MMDYN_MAX_EXPERTS];   /* expert log-variances */
  float* dmu[MMDYN_MAX_EXPERTS];        /* backward outputs (same shapes/strides) */
  float* dlv[MMDYN_MAX_EXPERTS];
  int ld[MMDYN_MAX_EXPERTS];            /* row stride of the expert tensors (heads are stored fused: [rows][2L]) */
  const float* dz[3];                   /* backward only: up to three [B][L] latent gradients of this pass (one per
                                           decoder that consumed z), summed by the kernel; null = none */
  float* zdst[3];                       /* forward only (revision 6): up to three further [B][L] destinations of this pass's z --
                                           its row block in the stacked input of each decoder that consumes it (the
                                           torch.cat of the subset passes, problems.py:478-529, without a copy launch);
                                           null = none */
  void* zpl[3];                         /* forward only (revision 6): the same row blocks as PLANE tensors (rows of [plane][L] bf16,
                                           the exact three-term split: mmdyn_split_planes) for a decoder whose first GEMM takes
                                           its operand already split; null = none */
} mmdyn_pass_experts;
/* P passes of [B][L].  with_prior=1 adds the universal N(0,1) expert first (vae.py:139, 321-328).
 * Outputs mu/logvar [P][B][L]; optional z = eps*exp(logvar/2)+mu; optional kl_sum[p] (double)
 * += -0.5*sum(1+lv-mu^2-e^lv).  eps added twice to each variance, as the reference does. */
/* mu / logvar / z (zdst, zpl): OUTPUTS; kl_sum: ACCUMULATOR (the caller zeroes it). */
int mmdyn_poe_fwd(const mmdyn_pass_experts* passes, const float* eps_noise, float* mu, float* logvar,
                  float* z, double* kl_sum, int with_prior, int P, int B, int L, void* stream);
/* upstream gradients: dz [P][B][L] (through z), g_mu / g_lv [P][B][L] (directly on the fused mu/logvar),
 * any may be null; kl_scale = kl_weight / B adds the KL term's gradient. */
/* dmu / dlv of the experts present in a pass: OUTPUTS (all B rows); an expert whose pointers are null in the pass is not touched. */
int mmdyn_poe_bwd(const mmdyn_pass_experts* passes, const float* eps_noise, const float* mu,
                  const float* logvar, const float* dz, const float* g_mu, const float* g_lv, float kl_scale,
                  int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream);
/* single-expert path (VAE, vae.py:81-88): reparametrisation and/or KL on mu/lv rows of stride ld */
int mmdyn_reparam_fwd(const float* mu, const float* lv, const float* eps_noise, float* z, double* kl_sum,
                      int B, int L, int ld, void* stream);
int mmdyn_reparam_bwd(const float* mu, const float* lv, const float* eps_noise, const float* dz,
                      float kl_scale, float* dmu, float* dlv, int B, int L, int ld, void* stream);

/* ---- ELBO reconstruction terms (problems.py:433-449) ----------------------------------------- */
/* sum over all elements of BCE-with-logits(x, t) added to *loss_sum (double); optional dlogit =
 * (sigmoid(x) - t) * grad_scale.  With `mask` ([B][mask_channels][H][W]; mask_channels = 1: broadcast over the
 * channels, = C: elementwise, the dataset's 3-channel segmentation mask) both logits and targets are multiplied by it
 * first (problems.py:445-447); any other channel count is MMDYN_ERR_SHAPE. */
/* dlogit: OUTPUT (a discarded pass of the grouped forms: zeros); loss_sum / loss_slots / unmasked_slots: ACCUMULATORS. */
int mmdyn_bce_logits(const float* logits, const float* target, const float* mask, float* dlogit,
                     double* loss_sum, int64_t n, int chw, int hw, int mask_channels, float grad_scale, void* stream);
/* The unmasked term for G decoder passes that share one target, in ONE launch: logits / dlogit [G][n], target [n];
 * pass g adds its sum to loss_slots[slot_of_group[g]] (a host array, copied by value into the launch: capturable);
 * a negative slot marks a discarded reconstruction (zero gradient, no loss).  The multi-subset ELBO of
 * problems.py:462-545 compares every subset's reconstruction of a modality with the same target. */
#define MMDYN_BCE_GROUPS_MAX 8
int mmdyn_bce_logits_groups(const float* logits, const float* target, float* dlogit, double* loss_slots,
                            const int* slot_of_group, int G, int64_t n, float grad_scale, void* stream);
/* The same launch with the loss mask of --mask-loss (problems.py:445-447, 684: torch.mul(recon, mask) against
 * torch.mul(target, mask)); mask [B][mask_channels][H][W] as in mmdyn_bce_logits (n = B*chw per pass).  unmasked_slots (may be
 * null) receives the plain sums next to the masked ones: the reference's perf_measure of the single-modality passes is
 * computed without the mask (problems.py:495-505). */
int mmdyn_bce_logits_groups_masked(const float* logits, const float* target, const float* mask, float* dlogit,
                                   double* loss_slots, double* unmasked_slots, const int* slot_of_group, int G, int64_t n,
                                   int chw, int hw, int mask_channels, float grad_scale, void* stream);
/* sum (r-t)^2 added to *loss_sum; dr = 2 (r-t) grad_scale */
int mmdyn_mse(const float* r, const float* t, float* dr, double* loss_sum, int64_t n, float grad_scale,
              void* stream);
/* The same for G passes against ONE target (F.mse_loss of the pose term, problems.py:439-443, for every pose-bearing subset of
 * the multi-subset ELBO): r / dr [G][n], t [n], loss_slots[slot_of_group[g]] += the sum of pass g.  One launch. */
int mmdyn_mse_groups(const float* r, const float* t, float* dr, double* loss_slots, const int* slot_of_group, int G, int64_t n,
                     float grad_scale, void* stream);
/* loss[0] = (sum_p bce[p] + pose_multiplier * mse[p] + kl_weight * kl[p]) / B; partial[p] likewise.
 * kl_weight_dev (here and in mmdyn_poe_bwd; may be null): one float in device memory that multiplies kl_weight /
 * kl_scale -- the annealed KL weight of problems.py:212-216 kept on the device, so that a captured launch serves every
 * epoch of the schedule. */
int mmdyn_elbo_assemble(const double* bce, const double* mse, const double* kl, float* loss, float* partials,
                        int P, int B, float kl_weight, float pose_multiplier, const float* kl_weight_dev, void* stream);

/* ---- per-sample ELBO (the reduce=False branch of problems.py:401-458; evaluation only, no gradients) -------- */
/* torch.sum(F.binary_cross_entropy_with_logits(recon, x, reduce=False), (1, 2, 3)) (problems.py:409-416, 445-452) for G decoder
 * passes against ONE target: logits [G][Bg][chw], target [Bg][chw], mask (may be null) [Bg][mask_channels][hw] as in
 * mmdyn_bce_logits_groups_masked; rows_out[slot_of_group[g]][b] += the sum over sample b of pass g, rows_out [n_slots][Bg] double
 * (the caller zeroes it; two passes may share a slot; a negative slot is a discarded pass; a slot >= n_slots is MMDYN_ERR_SHAPE).
 * unmasked_rows (with a mask; may be null) also receives the plain sums.  chw % 4 == 0, hw % 4 == 0.  The target / mask row of a
 * sample is read once for all G passes.  Element arithmetic identical to mmdyn_bce_logits_groups. */
int mmdyn_bce_logits_rows_groups(const float* logits, const float* target, const float* mask, int mask_channels, double* rows_out,
                                 double* unmasked_rows, const int* slot_of_group, int n_slots, int G, int Bg, int chw, int hw,
                                 void* stream);
/* torch.sum(F.mse_loss(r, t, reduce=False), 1) (problems.py:439-452, the pose term) for G passes against one target: r [G][Bg][n],
 * t [Bg][n], rows_out[slot_of_group[g]][b] += sum_n (r - t)^2.  Slots in [0, n_slots). */
int mmdyn_mse_rows_groups(const float* r, const float* t, double* rows_out, const int* slot_of_group, int n_slots, int G, int Bg,
                          int n, void* stream);
/* kl_rows[p][b] = -0.5 * sum_L (1 + logvar - mu^2 - exp(logvar)) of mu / logvar [P][B][L] (what mmdyn_poe_fwd wrote, or the heads of
 * a VAE with P = 1): the terms of problems.py:406, 429 kept per sample -- the reference adds the batch TOTAL to every row.  Same
 * element expression as the kl_sum of mmdyn_poe_fwd / mmdyn_reparam_fwd: the rows of pass p add up to kl_sum[p] to fp64 rounding. */
int mmdyn_kl_rows(const float* mu, const float* logvar, double* kl_rows, int P, int B, int L, void* stream);
/* partials[p][b] = bce_rows[p][b] + pose_multiplier * mse_rows[p][b] + kl_weight * KL, out[b] = sum_p partials[p][b]; tables [P][B]
 * double (any may be null = 0), out [B] and partials [P][B] (may be null) float.  kl_mode 0: KL = kl_sum[p], the batch total in
 * every row -- what the reference returns (problems.py:415-417, 455-456); kl_mode 1: KL = kl_rows[p][b].  No division by B in either
 * mode.  kl_weight_dev as in mmdyn_elbo_assemble. */
int mmdyn_elbo_assemble_rows(const double* bce_rows, const double* mse_rows, const double* kl_rows, const double* kl_sum, float* out,
                             float* partials, int P, int B, float kl_weight, float pose_multiplier, const float* kl_weight_dev,
                             int kl_mode, void* stream);

/* ---- mixed-modality batches: per-ROW modality availability (replaces MVAE.forward, vae.py:126-165, run once per modality
 * subset on a sub-batch: the dataset yields the availability per frame, utils/datasets.py) -------------------------------- */
/* An availability table is uint8 [B][MMDYN_MAX_EXPERTS] in device memory, 4-byte aligned (the kernels read one 32-bit word per
 * row): byte m != 0 = expert m (visual, tactile, pose, spare) is present in row b.  Its contents are never inspected on the host.
 *
 * mmdyn_poe_fwd with one table per pass: avail (host array of P device pointers; null, or a null entry = every row holds every
 * expert of the pass, which reproduces mmdyn_poe_fwd bit for bit).  Expert m takes part in row b iff passes[p].mu[m] != NULL and
 * avail[p][b][m] != 0.  Same arithmetic and order as mmdyn_poe_fwd, so a row is bitwise the result of a pass that holds that
 * row's subset; all outputs (mu, logvar, z, zdst, zpl, kl_sum) are kept.  An absent (row, expert) is not read: its words may hold
 * NaN / Inf.  A row without any expert is the prior alone.  A table needs with_prior = 1 (MMDYN_ERR_SHAPE otherwise: without the
 * prior such a row divides by zero, and finding it would need the table's contents); a misaligned table is MMDYN_ERR_SHAPE. */
int mmdyn_poe_fwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise, float* mu,
                        float* logvar, float* z, double* kl_sum, int with_prior, int P, int B, int L, void* stream);
/* mmdyn_poe_bwd with the same tables: present (row, expert) pairs get the gradient mmdyn_poe_bwd gives for the row's subset, bit
 * for bit; the dmu / dlv row of an absent pair is WRITTEN as exact zeros (the heads' weight-gradient GEMM reads it). */
int mmdyn_poe_bwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise, const float* mu,
                        const float* logvar, const float* dz, const float* g_mu, const float* g_lv, float kl_scale, int with_prior,
                        int P, int B, int L, const float* kl_weight_dev, void* stream);
/* The completed modality of a request (replaces a per-subset forward + a row scatter): out[b] = present(b) ? x[b] :
 * (logits ? sigmoid(recon[b]) : recon[b]) for [B][row_len] fp32 tensors, present(b) = x != NULL && (avail == NULL ||
 * avail[b][modality] != 0).  Present rows are copied bit for bit; 16-byte accesses where the pointers are 16-byte aligned, any
 * row_len (a quad that straddles two rows selects per element).  sigmoid(v) = 1 / (1 + expf(-v)). */
int mmdyn_complete_select(const float* x, const float* recon, const uint8_t* avail, int modality, float* out, int B, int row_len,
                          int logits, void* stream);
/* mmdyn_elbo_assemble_rows with a TARGET-availability table: slot p of bce_rows / mse_rows belongs to the target modality
 * bce_modality[p] / mse_modality[p] (host arrays of P ints, copied by value; negative = the slot always counts).  A (row, slot)
 * whose target modality is absent in that row is left out of partials / out and its table entry is overwritten with 0 (whatever
 * it held).  P <= MMDYN_MAX_PASSES.  Everything else as mmdyn_elbo_assemble_rows: one launch, like the assembly it stands in for. */
int mmdyn_elbo_assemble_rows_avail(double* bce_rows, double* mse_rows, const double* kl_rows, const double* kl_sum, float* out,
                                   float* partials, const uint8_t* avail, const int* bce_modality, const int* mse_modality, int P,
                                   int B, float kl_weight, float pose_multiplier, const float* kl_weight_dev, int kl_mode,
                                   void* stream);

/* ---- gradients of the weighted per-sample ELBO (training with per-sample weights) -----------------------------------------------
 * L = (1/B) sum_b w_b * row_b, where row_b is what mmdyn_elbo_assemble_rows returns for sample b: the reference's
 * (w * rows).sum() / B on its reduce=False branch (problems.py:415-417, 451-456; kl_mode 0: the batch-total KL sits in every row,
 * so it is weighted by sum_b w_b), or the same with each sample's own KL (kl_mode 1).  w: fp32 [B], any values; a weight is never
 * inspected -- NaN / Inf propagate (0 * NaN = NaN).  The backward of the step starts from three seeds (BCE, MSE, KL); each of the
 * launches below is the seed kernel with its scalar scale replaced by scale * weight-of-the-sample, the product formed as
 * (unweighted gradient) * w so that w = 1 gives the unweighted kernel's gradient bit for bit.  The loss sums these launches produce
 * are the UNWEIGHTED row tables of the section above; BatchNorm statistics are those of the unweighted batch.
 *
 * mmdyn_tconv_out3_bn_bce_rows with the gradient output: loss_rows / unmasked_rows as there (unweighted), dlogit [G*Bg][3][2Hi][2Wi]
 * = ((sigmoid(l) - t) * grad_scale) * w_rec[b]  (with a mask: (mk * (sigmoid(mk l) - mk t) * grad_scale) * w_rec[b]); a discarded
 * pass (slot < 0) gets a zero gradient and no loss.  w_rec [Bg] is read once per block.  dlogit and w_rec are required. */
int mmdyn_tconv_out3_bn_bce_rows_grad(const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                      const float* w, float* logits, int logits_group, const float* target, const float* mask,
                                      int mask_channels, float* dlogit, const float* w_rec, double* loss_rows, double* unmasked_rows,
                                      const int* slot_of_group, int n_slots, float grad_scale, int G, int Bg, int Hi, int Wi, int b16,
                                      void* stream);
/* mmdyn_bce_logits_rows_groups with dlogit [G][Bg][chw] = ((sigmoid - t) * grad_scale) * w_rec[b] in the same pass over the logits
 * (zeros for a pass with a negative slot); the target / mask row of a sample is read once for all G passes.  G * Bg * chw < 2^31
 * (MMDYN_ERR_RANGE). */
int mmdyn_bce_logits_rows_groups_grad(const float* logits, const float* target, const float* mask, int mask_channels, float* dlogit,
                                      const float* w_rec, double* rows_out, double* unmasked_rows, const int* slot_of_group,
                                      int n_slots, float grad_scale, int G, int Bg, int chw, int hw, void* stream);
/* mmdyn_mse_rows_groups with dr [G][Bg][n] = (2 (r - t) * grad_scale) * w_rec[b]. */
int mmdyn_mse_rows_groups_grad(const float* r, const float* t, float* dr, const float* w_rec, double* rows_out,
                               const int* slot_of_group, int n_slots, float grad_scale, int G, int Bg, int n, void* stream);
/* mmdyn_poe_bwd / mmdyn_reparam_bwd with the KL scale of row b = kl_scale * w_kl[b] (w_kl fp32 [B]; kl_weight_dev still multiplies).
 * kl_mode 1 passes w_kl = w; kl_mode 0 passes the vector filled with sum_b w_b that mmdyn_elbo_assemble_weighted writes.  dz arrives
 * weighted through the decoders and is not scaled again.  With w_kl = 1 the results equal the unweighted kernels' bit for bit. */
int mmdyn_poe_bwd_weighted(const mmdyn_pass_experts* passes, const float* eps_noise, const float* mu, const float* logvar,
                           const float* dz, const float* g_mu, const float* g_lv, float kl_scale, const float* w_kl, int with_prior,
                           int P, int B, int L, const float* kl_weight_dev, void* stream);
int mmdyn_reparam_bwd_weighted(const float* mu, const float* lv, const float* eps_noise, const float* dz, float kl_scale,
                               const float* w_kl, float* dmu, float* dlv, int B, int L, int ld, void* stream);
/* From the fp64 row tables [P][B] (any may be null = 0), kl_sum [P] and w [B]:
 *   wpartials[p] = (sum_b w_b (bce[p][b] + pose_multiplier mse[p][b]) + kl_weight * (kl_mode ? sum_b w_b kl_rows[p][b]
 *                                                                                           : (sum_b w_b) kl_sum[p])) / B,
 *   loss[0] = sum_p wpartials[p]   (fp32; wpartials may be null),
 * plus the unweighted out [B] / partials [P][B] of mmdyn_elbo_assemble_rows in the same kl_mode (either may be null) and, when
 * w_sum_out is non-null, w_sum_out[b] = (float)sum_b w_b for every b.  fp64 accumulation in a fixed order by one block, no atomics:
 * the same bits in every run.  P <= MMDYN_MAX_PASSES.  kl_weight_dev as in mmdyn_elbo_assemble. */
int mmdyn_elbo_assemble_weighted(const double* bce_rows, const double* mse_rows, const double* kl_rows, const double* kl_sum,
                                 const float* w, float* loss, float* wpartials, float* out, float* partials, float* w_sum_out, int P,
                                 int B, float kl_weight, float pose_multiplier, const float* kl_weight_dev, int kl_mode, void* stream);

/* ---- the training step on a mixed-modality batch: per-row INPUT availability in the PoE, per-row TARGET availability in the loss ---
 * L = (1/B) sum_p sum_b w_b * [ sum_{m in pass p, target m present in row b} rec_m(p, b) + kl_weight * KL(p, b) ]; the division stays
 * by B.  Every row passes through every encoder and decoder (BatchNorm statistics are those of the whole batch); only the PoE leaves
 * an absent (row, expert) unread, and only the loss leaves an absent (row, target) out.
 *
 * mmdyn_poe_bwd with BOTH the tables of mmdyn_poe_bwd_avail and the row weights of mmdyn_poe_bwd_weighted (the arguments are the
 * union of the two; w_kl is required).  With avail null (or every entry null) the results are mmdyn_poe_bwd_weighted's bit for bit,
 * with w_kl = 1 they are mmdyn_poe_bwd_avail's.  Any L: with L % 64 != 0 a wavefront spans rows and the per-expert branch diverges,
 * each lane follows its own row's word. */
int mmdyn_poe_bwd_avail_weighted(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise, const float* mu,
                                 const float* logvar, const float* dz, const float* g_mu, const float* g_lv, float kl_scale,
                                 const float* w_kl, int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream);
/* The weight vectors of the three gradient seeds (visual BCE, tactile BCE, pose MSE) in one launch:
 *   w_term[m][b] = tavail[b][m] != 0 ? (w ? w[b] : 1.f) : 0.f,  m = 0, 1, 2;   w_term: [3][B] float, OUTPUT.
 * tavail: a TARGET-availability table (null = every target present); w: [B] float or null.  A select, never a product: the weight of
 * a row whose target is absent (it may be NaN) reaches nothing.  One 32-bit word per row; a misaligned table or B <= 0:
 * MMDYN_ERR_SHAPE; w_term null: MMDYN_ERR_NULL. */
int mmdyn_term_weights(const uint8_t* tavail, const float* w, float* w_term, int B, void* stream);
/* mmdyn_elbo_assemble_weighted with one [P][B] double table per TERM -- bce_v_rows (visual BCE), bce_t_rows (tactile BCE), mse_rows
 * (pose MSE); any may be null = 0 -- and the target-availability table tavail (null = every target present).  A (row, term) whose
 * target is absent is left out of loss / wpartials / out / partials by selection and its table entries are overwritten with 0
 * (the tables are OUTPUTS for those entries), as in mmdyn_elbo_assemble_rows_avail.  The KL counts for every row.  w null = 1.
 * Also written (either may be null): present [3] double, the number of rows that hold target m; term_sums [3][P] double, the
 * UNWEIGHTED sum of term m's table over the rows that hold its target.  Everything else -- kl_mode, w_sum_out, kl_weight_dev, the
 * fixed-order fp64 accumulation by one block without atomics -- as mmdyn_elbo_assemble_weighted: with tavail null and w given the
 * results are its bits on the table bce_v_rows + bce_t_rows.  loss null: MMDYN_ERR_NULL; P > MMDYN_MAX_PASSES, a misaligned table,
 * or bce_v_rows == bce_t_rows (non-null): MMDYN_ERR_SHAPE. */
int mmdyn_elbo_assemble_avail_weighted(double* bce_v_rows, double* bce_t_rows, double* mse_rows, const double* kl_rows,
                                       const double* kl_sum, const float* w, const uint8_t* tavail, float* loss, float* wpartials,
                                       float* out, float* partials, float* w_sum_out, double* present, double* term_sums, int P, int B,
                                       float kl_weight, float pose_multiplier, const float* kl_weight_dev, int kl_mode, void* stream);

/* ---- importance-weighted K-sample bound (evaluation only; no reference op: the reference scores a sample with one draw and the
 * analytic KL, problems.py:401-458) -------------------------------------------------------------------------------------------------
 * L_K(x) = log (1/K) sum_k p(x|z_k) p(z_k) / q(z_k|x), z_k ~ q(z|x) (Burda et al., "Importance Weighted Autoencoders"), per request
 * row b from K draws of ONE posterior: the ELBO at K = 1, tightening towards log p(x) as K grows.  The two entry points bracket the
 * decoders (run on K * B rows) and the row kernels above (G = K passes against one target, slots 0..K-1 of [K][B] tables).
 *
 * The K draws of every row and the density ratio of each:
 *   z[k][b][l]  = eps[k][b][l] * exp(lv[b][l] / 2) + mu[b][l]   -- the fp32 expression of mmdyn_poe_fwd / mmdyn_reparam_fwd, in the
 *                 same order: the same mu, lv, eps give the same bits;
 *   ratio[k][b] = log q(z_k|x) - log p(z_k) = sum_l 0.5 * (z^2 - eps^2 - lv)   (the 2 pi terms cancel), evaluated in fp64 from the fp32
 *                 z, eps and lv, so it belongs to the z the decoders read.  E_q[ratio] is the analytic KL of mmdyn_kl_rows.
 * mu / lv: rows of stride ld >= L (the [B][L] outputs of mmdyn_poe_fwd, or the [B][2L] heads of a VAE); eps: [K][B][L], read;
 * z: [K][B][L], OUTPUT; ratio: [K][B] double, OUTPUT (written, not accumulated: no zeroing).  One wavefront per (k, b) row, 16-byte
 * lane accesses when L % 4 == 0, ld % 4 == 0 and the four pointers are 16-byte aligned; the fp64 sum runs in a fixed order without
 * atomics: the same bits in every run.  K * B * L >= 2^31: MMDYN_ERR_RANGE. */
int mmdyn_iw_latent(const float* mu, const float* lv, int ld, const float* eps, float* z, double* ratio, int K, int B, int L,
                    void* stream);
/* The bound from the row tables:
 *   log_w[k][b] = -(bce_rows[0][k][b] + bce_rows[1][k][b] + pose_multiplier * mse_rows[k][b]) - kl_weight * ratio[k][b],
 *   out[b]      = -(logsumexp_k log_w[k][b] - log K)            a loss, the sign of mmdyn_elbo_assemble_rows' out; at K = 1 exactly
 *                                                               the fp32 rounding of rec_0 + kl_weight * ratio_0,
 *   ess[b]      = exp(2 lse_k(log_w) - lse_k(2 log_w))          the effective sample size of the weights, in [1, K].
 * bce_rows: [n_bce][K][B] double, n_bce <= 2 (slot 0 = visual, 1 = tactile), may be null; mse_rows: [K][B] double or null; ratio:
 * [K][B] double, required.  tavail (may be null): a TARGET-availability table as in mmdyn_elbo_assemble_rows_avail -- bce slot s
 * belongs to modality s, mse_rows to modality 2; a (row, term) whose target is absent adds nothing to any log_w[k][b] and its K table
 * entries are overwritten with 0 (so bce_rows / mse_rows are OUTPUTS for those entries and read-only elsewhere).  out: [B] float,
 * OUTPUT; ess: [B] float, OUTPUT, may be null; log_w: [K][B] double, OUTPUT, may be null.  Max-subtracted log-sum-exp in fp64, one
 * thread per row b walking k.  A log_w of -inf is a zero weight; a row whose weights are all zero gets out = +inf and ess = NaN; NaN
 * propagates to out and ess; nothing is inspected on the host.  kl_weight_dev as in mmdyn_elbo_assemble.  n_bce outside [0, 2] or a
 * misaligned table: MMDYN_ERR_SHAPE. */
int mmdyn_iw_assemble_rows(double* bce_rows, double* mse_rows, const double* ratio, const uint8_t* tavail, float* out, float* ess,
                           double* log_w, int n_bce, int K, int B, float pose_multiplier, float kl_weight, const float* kl_weight_dev,
                           void* stream);

/* ---- multi-step rollout of the one-step dynamics model (replaces, in a loop, MVAE.forward, vae.py:126-165, followed by the
 * sigmoid that takes the image logits to image space, problems.py:616-626: the reference never feeds a prediction back) ---------
 * One launch turns the decoder outputs of step t into the inputs of step t + 1, for up to MMDYN_FEED_GROUPS tensors (visual
 * image, tactile image, pose) at once:
 *   out[g][b][i] = (obs[g] && (!obs_avail || obs_avail[b][column[g]])) ? obs[g][b][i]
 *                                                                    : (logits[g] ? 1 / (1 + expf(-r)) : r),  r = recon[g][b][i],
 * every tensor fp32 [B][row_len[g]].  obs_avail: an availability table as above (uint8 [B][MMDYN_MAX_EXPERTS], 4-byte aligned,
 * MMDYN_ERR_SHAPE otherwise; null = every row of every given obs is observed); column[g] is the table byte of group g.  An observed
 * row is copied bit for bit; the side that is not taken is not loaded and may hold NaN / Inf.  Each group's output has the bits of
 * mmdyn_complete_select(obs[g], recon[g], obs_avail, column[g], out[g], B, row_len[g], logits[g]) -- same expression, same access
 * scheme: 16-byte accesses where the three pointers of the group are 16-byte aligned, element by element otherwise, any row_len
 * (a quad that straddles two rows selects per element).  A block works on one group and the grid is divided between the groups
 * by their quad counts.  No LDS, no atomics, no workspace.
 * Checked on the host before the launch: groups, or recon / out of a group < G, null: MMDYN_ERR_NULL; G outside
 * [1, MMDYN_FEED_GROUPS], B < 1, a row_len < 1, a column outside [0, MMDYN_MAX_EXPERTS), a misaligned table, or an out[g] that
 * overlaps recon[g] or obs[g]: MMDYN_ERR_SHAPE; B * row_len[g] >= 2^31: MMDYN_ERR_RANGE.  The struct is read during the call only.
 * Added without touching an existing signature or workspace: the revision stays 6. */
#define MMDYN_FEED_GROUPS 4
typedef struct {
  const float* recon[MMDYN_FEED_GROUPS];  /* [B][row_len[g]]: the step's decoder output (image logits / pose decoder output) */
  const float* obs[MMDYN_FEED_GROUPS];    /* observed next frame, same shape; null: nothing observed in this group */
  float* out[MMDYN_FEED_GROUPS];          /* next state = trajectory slot, same shape */
  int row_len[MMDYN_FEED_GROUPS];
  int logits[MMDYN_FEED_GROUPS];          /* != 0: recon holds logits, the state is their sigmoid */
  int column[MMDYN_FEED_GROUPS];          /* availability-table byte of the group */
} mmdyn_feed_groups;
int mmdyn_rollout_feed(const mmdyn_feed_groups* groups, int G, const uint8_t* obs_avail, int B, void* stream);

/* ---- ensemble rollout: N sampled trajectories per request row, their statistics from the same read (the reference draws one z
 * per forward, vae.py:126-165, and has no rollout) -------------------------------------------------------------------------
 * The feed of N * B trajectory rows, sample-major (row n * B + b is trajectory n of request row b), under observations that
 * exist once per request row, for up to MMDYN_FEED_GROUPS tensors at once.  With p = logits[g] ? 1 / (1 + expf(-r)) : r,
 * r = recon[g][n * B + b][i], and observed(g, b) = obs[g] && (!obs_avail || obs_avail[b][column[g]]) on the B-row table:
 *   out[g][n * B + b][i] = observed(g, b) ? obs[g][b][i] : p            the bits of mmdyn_rollout_feed on the same N * B rows with
 *                                                                        obs[g] and the table repeated N times, for every N;
 *   mean[g][b][i]        = (1 / N) sum_n p                               of the PREDICTION, observed or not;
 *   var[g][b][i]         = (1 / N) sum_n (p - mean)^2                    the population variance; N = 1: 0;
 *   spread[g][b]        += sum_i var[g][b][i]                            the fp32 values as written, widened; an ACCUMULATOR.
 * The statistics are accumulated in fp64 in n order around c = p_0: d_n = p_n - c, S1 = sum d_n, S2 = sum d_n^2,
 * mean = (float)(c + S1 / N), var = (float)max(0, (S2 - S1^2 / N) / N): mean within 2^-23 max_n |p_n| and var within 2^-22 relative
 * (+ 2^-126) of the exact values; N identical samples give var == 0 and mean == p exactly; a NaN sample makes the element's mean and
 * var NaN and nothing else.  spread is added by fp64 atomics (one per wavefront where its elements lie in one row): equal only to
 * rounding between runs; everything else has the same bits in every run.
 * A thread owns one quad (or element) of the [B][row_len] plane and walks n: every recon element is loaded exactly once (always:
 * the statistics need it), the obs quad once before the walk and only where it is taken -- an obs row of an unobserved (row, group)
 * is never loaded and may hold NaN / Inf.  16-byte accesses where recon, obs, out, mean and var of the group are 16-byte aligned and
 * B * row_len % 4 == 0 (the sample stride keeps the alignment), element by element otherwise, any row_len (a quad that straddles
 * rows selects per element).  A block works on one group.  No LDS beyond the wave reduction, no workspace.  out, mean and var are
 * OUTPUTS: every element written, none read.
 * Checked on the host before the launch: groups, or recon / out / mean of a group < G, null: MMDYN_ERR_NULL; G outside
 * [1, MMDYN_FEED_GROUPS], N < 1, B < 1, a row_len < 1, a column outside [0, MMDYN_MAX_EXPERTS), a misaligned table, spread without
 * var (or not 8-byte aligned), or an out / mean / var / spread of any group that overlaps the recon or obs of ANY group < G, the table
 * or another output of the launch: MMDYN_ERR_SHAPE; N * B * row_len[g] >= 2^31: MMDYN_ERR_RANGE.  The struct is read during the call
 * only.  Added without touching an existing signature or workspace: the revision stays 6. */
typedef struct {
  const float* recon[MMDYN_FEED_GROUPS];  /* [N * B][row_len[g]], sample-major: the step's decoder output */
  const float* obs[MMDYN_FEED_GROUPS];    /* [B][row_len[g]]: one observation per request row; null: nothing observed in this group */
  float* out[MMDYN_FEED_GROUPS];          /* [N * B][row_len[g]]: next state = trajectory slot */
  float* mean[MMDYN_FEED_GROUPS];         /* [B][row_len[g]], required */
  float* var[MMDYN_FEED_GROUPS];          /* [B][row_len[g]], may be null */
  double* spread[MMDYN_FEED_GROUPS];      /* [B], may be null; the caller zeroes it; needs var */
  int row_len[MMDYN_FEED_GROUPS];
  int logits[MMDYN_FEED_GROUPS];          /* != 0: recon holds logits, the state is their sigmoid */
  int column[MMDYN_FEED_GROUPS];          /* availability-table byte of the group */
} mmdyn_ensemble_groups;
int mmdyn_ensemble_feed(const mmdyn_ensemble_groups* groups, int G, const uint8_t* obs_avail, int N, int B, void* stream);

/* mmdyn_ensemble_quantiles: Q order statistics per element of the ensemble's prediction, for up to MMDYN_FEED_GROUPS tensors in one
 * launch (MVAEInference.rollout(samples=N, quantiles=...): the prediction band the mean and the variance do not give for a squashed
 * pixel).  src[g] is fp32 [N][plane], plane = B * row_len[g], sample-major -- the layout of mmdyn_ensemble_groups.recon --, and
 * p_n = logits[g] ? 1 / (1 + expf(-src)) : src, the bits mmdyn_ensemble_feed writes into out for the same element.  For element e
 * let s_0 <= ... <= s_{N-1} be the N values p_n[e] in ascending order of the fp32 `<`, and hi = min(lo[j] + 1, N - 1).  Then
 *   out[g][j][e] = s_lo[j]                                                      where frac[j] == 0: no arithmetic, so +-Inf samples
 *                                                                               are ordinary values;
 *   out[g][j][e] = (float)((double)s_lo + frac[j] * ((double)s_hi - (double)s_lo))   otherwise: the difference, the product and the
 *                                                                               sum each rounded on their own in fp64, then ONE
 *                                                                               rounding to fp32.
 * With lo = floor(h), frac = h - lo, h = q * (N - 1) -- formed by the CALLER, the kernel never sees q -- this is the `linear`
 * quantile of numpy / torch.quantile; a restatement made of a sort and single fp64 operations has the same bits.  Values that
 * compare equal are interchangeable: only the SIGN OF A ZERO result is unspecified (-0.0 == +0.0).  A NaN among the N samples of an
 * element makes all Q outputs of THAT element NaN and nothing else (the rule of mean / var).  No atomics: the same bits in every run.
 * One wavefront per block works on chunks of 64 consecutive elements: the chunk's N x 64 values go through LDS once (N rounded up
 * to four, times 256 bytes: 32 KB at MMDYN_QUANTILE_N_MAX), each lane then ranks the samples of its own element (sample n has rank
 * #{m: p_m < p_n or (p_m == p_n and m < n)}) and keeps those of rank lo[j] and hi.  Every src element is loaded from global memory
 * exactly once; 16-byte accesses where src[g] and out[g] are 16-byte aligned and plane % 4 == 0, element by element otherwise.  A
 * block works on one group.  No workspace, no scratch; out is an OUTPUT: every element written, none read.
 * Checked on the host before the launch: groups, or src / out of a group < G, null: MMDYN_ERR_NULL; G outside
 * [1, MMDYN_FEED_GROUPS], Q outside [1, MMDYN_QUANTILES_MAX], N < 1, B < 1, a row_len < 1, a lo[j] outside [0, N), a frac[j] outside
 * [0, 1) or NaN (j < Q), or an out[g] that overlaps the src of ANY group < G or the out of another: MMDYN_ERR_SHAPE;
 * N > MMDYN_QUANTILE_N_MAX, N * plane >= 2^31 or Q * plane >= 2^31: MMDYN_ERR_RANGE.  The struct is read during the call only: lo and
 * frac travel to the kernel by value.  Added without touching an existing signature or workspace: the revision stays 6. */
#define MMDYN_QUANTILES_MAX 8
#define MMDYN_QUANTILE_N_MAX 128
typedef struct {
  const float* src[MMDYN_FEED_GROUPS];    /* [N][B * row_len[g]], sample-major */
  float* out[MMDYN_FEED_GROUPS];          /* [Q][B * row_len[g]] */
  int row_len[MMDYN_FEED_GROUPS];
  int logits[MMDYN_FEED_GROUPS];          /* != 0: src holds logits, the quantiles are those of their sigmoid */
  int lo[MMDYN_QUANTILES_MAX];            /* index of the lower order statistic of quantile j */
  double frac[MMDYN_QUANTILES_MAX];       /* weight of the upper one, in [0, 1) */
} mmdyn_quantile_groups;
int mmdyn_ensemble_quantiles(const mmdyn_quantile_groups* groups, int G, int Q, int N, int B, void* stream);

/* ---- candidate conditions: N conditions scored per row, the best one picked on the device (the reference has no such operation:
 * with vae.py:126-165 a caller would run MVAE.forward once per candidate and take the argmin of the losses of problems.py:473-546
 * on the host) --------------------------------------------------------------------------------------------------------------
 * mmdyn_plan_select: the cost table and each row's winner from the row tables of the N * B (candidate, row) passes:
 *   c[n][b]    = ((bce_rows[0][n][b] + bce_rows[1][n][b]) + pose_multiplier * mse_rows[n][b]) + kl_weight * kl_rows[n][b]
 *                in fp64, in exactly this order, every product and every sum rounded to nearest on its own (no fused multiply-add);
 *   cost[n][b] = (float)c[n][b];  best[b] = the n of the smallest c[n][b];  best_cost[b] = (float)c[best[b]][b].
 * Selection rules, on the fp64 value: the smallest cost wins; equal costs: the lowest n; a NaN cost never wins; +Inf / -Inf are
 * ordinary values (+Inf loses to every finite cost, -Inf wins).  All N costs of a row NaN: best[b] = -1, best_cost[b] = NaN, the
 * row of best_cond is NaN (best_idx[b] = -1).
 * bce_rows: [2][N][B] double (slot 0 = visual, 1 = tactile), may be null; mse_rows: [N][B] double or null; kl_rows: [N][B] double,
 * required.  A table that is null enters as +0.0.  tavail (may be null): a TARGET-availability table as in
 * mmdyn_iw_assemble_rows -- bce slot s belongs to modality s, mse_rows to modality 2; a (row, term) whose target is absent enters
 * as +0.0 for every n and its N table entries are overwritten with 0 (so bce_rows / mse_rows are OUTPUTS for those entries and
 * read-only elsewhere).  Candidates, candidate-major, exactly one kind (MMDYN_ERR_NULL otherwise), with the output of that kind:
 *   cand [N * B][cd] float  -> best_cond [B][cd] float = cand[best[b] * B + b];
 *   cand_idx [N * B] int64  -> best_idx [B] int64 = cand_idx[best[b] * B + b]  (cd is not used).
 * cost: [N][B] float; best: [B] int; best_cost: [B] float; all OUTPUTS.  kl_weight_dev as in mmdyn_elbo_assemble.  One thread per
 * row b walking n; no atomics: the same bits in every run.  N < 1, B < 1, cd < 1 or a misaligned table: MMDYN_ERR_SHAPE;
 * N * B * cd >= 2^31: MMDYN_ERR_RANGE. */
int mmdyn_plan_select(double* bce_rows, double* mse_rows, const double* kl_rows, const uint8_t* tavail, const float* cand,
                      const int64_t* cand_idx, int cd, float* cost, int* best, float* best_cost, float* best_cond,
                      int64_t* best_idx, int N, int B, float pose_multiplier, float kl_weight, const float* kl_weight_dev,
                      void* stream);
/* mmdyn_gather_best: the winner's rows out of the candidate-major outputs, for up to MMDYN_FEED_GROUPS tensors in one launch:
 *   out[g][b][i] = f(src[g][best[b] * B + b][i]),  f(r) = logits[g] ? 1 / (1 + expf(-r)) : r,
 * src[g]: fp32 [N * B][row_len[g]], out[g]: fp32 [B][row_len[g]].  The element scheme of mmdyn_rollout_feed (16-byte accesses where
 * src[g] and out[g] are 16-byte aligned, element by element otherwise, any row_len; a block works on one group), so a row has the
 * bits of mmdyn_complete_select(NULL, src[g] + (best[b] * B + b) * row_len[g], ...) on that row.  best[b] == -1 (mmdyn_plan_select:
 * every cost NaN): the row is filled with NaN and nothing is read; an index outside [-1, N) is treated the same way -- it never
 * causes an access out of bounds.  Rows that are not taken are not loaded and may hold NaN / Inf.  No LDS, no atomics.
 * Checked on the host: groups, best, or src / out of a group < G, null: MMDYN_ERR_NULL; G outside [1, MMDYN_FEED_GROUPS], N < 1,
 * B < 1, a row_len < 1, or an out[g] that overlaps best, the src of ANY group < G or the out of another group < G:
 * MMDYN_ERR_SHAPE; N * B * row_len[g] >= 2^31: MMDYN_ERR_RANGE.
 * The struct is read during the call only.  Both added without touching an existing signature or workspace: the revision stays 6. */
typedef struct {
  const float* src[MMDYN_FEED_GROUPS];    /* [N * B][row_len[g]], candidate-major: the decoder outputs of every (candidate, row) */
  float* out[MMDYN_FEED_GROUPS];          /* [B][row_len[g]]: the winner's row of each b */
  int row_len[MMDYN_FEED_GROUPS];
  int logits[MMDYN_FEED_GROUPS];          /* != 0: src holds logits, out their sigmoid */
} mmdyn_gather_groups;
int mmdyn_gather_best(const mmdyn_gather_groups* groups, int G, const int* best, int N, int B, void* stream);

/* ---- candidate condition SEQUENCES over T steps (MVAEInference.plan_rollout: N candidate sequences per row rolled out open loop,
 * the best one picked on the device; the reference has no such operation) ---------------------------------------------------
 * mmdyn_plan_select_steps: the step costs, the weighted total and each row's winner from the row tables of the Tg scored steps:
 *   c[t][n][b]         = ((bce_rows[0][t][n][b] + bce_rows[1][t][n][b]) + pose_multiplier * mse_rows[t][n][b])
 *                        + kl_weight * kl_rows[t][n][b]                  -- the cost of mmdyn_plan_select, the same function;
 *   step_cost[t][n][b] = (float)c[t][n][b];
 *   total[n][b]        = w[0] * c[0][n][b] + w[1] * c[1][n][b] + ... in fp64, t ascending, w[t] = (double)step_weight[t]; every
 *                        product and every sum rounded to nearest on its own (no fused multiply-add), the first term starts the
 *                        sum; step_weight null: the plain sum c[0] + c[1] + ..., with no multiplication;
 *   cost[n][b]         = (float)total[n][b];  best[b] = the n of the smallest total;  best_cost[b] = (float)total[best[b]][b].
 * Selection on the fp64 total by the rules of mmdyn_plan_select: the smallest wins; equal totals: the lowest n; a NaN total never
 * wins (a NaN in one step makes the total NaN); +Inf / -Inf are ordinary values.  All N totals of a row NaN: best[b] = -1,
 * best_cost[b] = NaN, the T rows of best_cond NaN (best_idx -1).
 * Tg is 1 (a final goal: the tables hold the one scored step) or T (every step scored).  bce_rows: [2][Tg][N][B] double or null;
 * mse_rows: [Tg][N][B] double or null; kl_rows: [Tg][N][B] double, required; a null table enters as +0.0.  tavail (may be null):
 * [Tg][B][4] bytes, the TARGET-availability table of each scored step; an absent (step, row, term) enters as +0.0 for every n and
 * its N table entries are overwritten with 0.  step_weight: [Tg] float in DEVICE memory or null; the values are not looked at on
 * the host (NaN / Inf propagate into the totals).  Candidates, step-major and candidate-major, exactly one kind:
 *   cand [T][N * B][cd] float  -> best_cond [B][T][cd] float = cand[t][best[b] * B + b] for all T steps;
 *   cand_idx [T][N * B] int64  -> best_idx [B][T] int64      (cd is not used).
 * top / top_cost (both or neither): [K][B] int / float, K in [1, MMDYN_PLAN_TOP_MAX]: the K smallest totals of each row in
 * ascending order under the same rules -- equal totals in n order, a NaN total never listed; entries past the number of non-NaN
 * candidates are -1 / NaN; top[0][b] == best[b].  cost [N][B], step_cost [Tg][N][B], best [B], best_cost [B]: OUTPUTS.
 * kl_weight_dev as in mmdyn_elbo_assemble.  One thread per row b; no atomics, no LDS: the same bits in every run.
 * With Tg = T = 1 and step_weight null, cost / best / best_cost / best_cond (best_idx) have the bits of mmdyn_plan_select on the
 * same tables, and step_cost those of cost.
 * Checked on the host: kl_rows, cost, step_cost, best or best_cost null, not exactly one kind of candidates with its output, or
 * top without top_cost (or the reverse): MMDYN_ERR_NULL; N, B, T, Tg or cd < 1, Tg neither 1 nor T, K outside
 * [1, MMDYN_PLAN_TOP_MAX] with top given, or a misaligned table: MMDYN_ERR_SHAPE; T * N * B * cd >= 2^31: MMDYN_ERR_RANGE. */
#define MMDYN_PLAN_TOP_MAX 8
int mmdyn_plan_select_steps(double* bce_rows, double* mse_rows, const double* kl_rows, const uint8_t* tavail,
                            const float* step_weight, const float* cand, const int64_t* cand_idx, int cd, float* cost,
                            float* step_cost, int* best, float* best_cost, float* best_cond, int64_t* best_idx, int* top,
                            float* top_cost, int K, int N, int B, int T, int Tg, float pose_multiplier, float kl_weight,
                            const float* kl_weight_dev, void* stream);
/* mmdyn_gather_best_steps: the winner's rows of all T steps out of step-major, candidate-major tensors, in one launch:
 *   out[g][t][b][i] = f(src[g][t][best[b] * B + b][i]),  f as in mmdyn_gather_best,
 * src[g]: fp32 [T][N * B][row_len[g]], out[g]: fp32 [T][B][row_len[g]] (mmdyn_gather_groups with these shapes).  The element scheme
 * of mmdyn_gather_best on every step slice (16-byte accesses where the slice's src and out are 16-byte aligned, element by element
 * otherwise; a block works on one group and one step at a time; a row whose index lies outside [0, N) is filled with NaN and
 * reads nothing): the result has the bits of T mmdyn_gather_best calls on the slices src[g] + t * N * B * row_len[g], out[g] +
 * t * B * row_len[g].  No LDS, no atomics.
 * Checked on the host: groups, best, or src / out of a group < G, null: MMDYN_ERR_NULL; G outside [1, MMDYN_FEED_GROUPS], N, B or
 * T < 1, a row_len < 1, or an out[g] that overlaps best, the src of ANY group < G or the out of another group < G:
 * MMDYN_ERR_SHAPE; T * N * B * row_len[g] >= 2^31: MMDYN_ERR_RANGE.
 * Both added without touching an existing signature or workspace: the revision stays 6. */
int mmdyn_gather_best_steps(const mmdyn_gather_groups* groups, int G, const int* best, int N, int B, int T, void* stream);

/* ---- iterative refinement of a candidate distribution (MVAEInference.plan_refine: the cross-entropy method on the horizon
 * planner -- sample N condition sequences per row from N(mean, std^2), roll them out, refit mean / std to the K best, repeat; the
 * reference has no such operation) ----------------------------------------------------------------------------------------
 * mmdyn_plan_sample: the candidates of one iteration, in the layout mmdyn_plan_select_steps and the planner's steps read:
 *   cand[t][n * B + b][d] = clamp(n == 0 ? (keep && keep[b][t][d] is no NaN ? keep[b][t][d] : mean[b][t][d])
 *                                        : mean[b][t][d] + std[b][t][d] * eps[n][b][t][d]),
 * the product rounded to fp32, then the sum rounded to fp32 (no fused multiply-add); clamp(c) = c < lo[d] ? lo[d] : (c > hi[d] ?
 * hi[d] : c) with bounds, c without -- a NaN stays a NaN.  Slot n = 0 is the incumbent (the best sequence of the previous
 * iteration, or the mean): its eps is never read.  mean, std: [B][T][cd]; eps: [N][B][T][cd]; keep: [B][T][cd] or null; lo, hi:
 * [cd], both or neither; cand: [T][N * B][cd], an OUTPUT that overlaps no input.  All fp32.  One element per thread, or 16-byte
 * accesses where cd % 4 == 0 and every pointer is 16-byte aligned (the same values either way).  No LDS, no atomics.
 * Checked on the host: mean, std, eps or cand null, or one bound without the other: MMDYN_ERR_NULL; N, B, T or cd < 1, or cand
 * overlapping an input: MMDYN_ERR_SHAPE; N * B * T * cd >= 2^31: MMDYN_ERR_RANGE.
 *
 * mmdyn_plan_refit: the elites of every row and the distribution refitted to them.  cost: [N][B] float, as
 * mmdyn_plan_select_steps writes it; cand: [T][N * B][cd]; mean_in, std_in: [B][T][cd].  Per row b:
 *   candidate n is an ELITE iff cost[n][b] is no NaN and fewer than K candidates m have cost[m][b] < cost[n][b], or cost[m][b] ==
 *   cost[n][b] with m < n: the K smallest, ties to the lower n, a NaN never, +Inf / -Inf ordinary values (the rules of
 *   mmdyn_plan_select, on the fp32 cost).  K' = the number of elites (K' < K when fewer than K costs are no NaN).
 *   K' == 0: mean_out = mean_in, std_out = std_in, bit for bit.  Otherwise per element (t, d), in fp64, over the elites in
 *   ascending n, every sum, product, quotient and root rounded on its own (no fused multiply-add):
 *     m = (sum (double)c_n) / K';  v = (sum ((double)c_n - m)^2) / K';  s = sqrt(v);
 *     mean_out = (float)((double)alpha * (double)mean_in + (1.0 - (double)alpha) * m);
 *     std_out  = fmaxf((float)((double)alpha * (double)std_in + (1.0 - (double)alpha) * s), std_min).
 * mean_out, std_out: [B][T][cd], each may be exactly its input; elite (may be null): [N][B] bytes, 1 = elite; count (may be null):
 * [B] int = K'.  One block of 256 threads per row: the cost column and the flags in LDS (MMDYN_REFIT_N_MAX * 5 bytes), ranks by
 * counting, one fixed summation order; no atomics: the same bits in every run.  Candidates that are no elites are not loaded.
 * Checked on the host: cost, cand, mean_in, std_in, mean_out or std_out null: MMDYN_ERR_NULL; B, T or cd < 1, N outside
 * [1, MMDYN_REFIT_N_MAX], K outside [1, N], alpha outside [0, 1), std_min < 0 (or either a NaN), or an output that overlaps
 * anything but its own input: MMDYN_ERR_SHAPE; N * B * T * cd >= 2^31: MMDYN_ERR_RANGE.
 * Both added without touching an existing signature or workspace: the revision stays 6. */
#define MMDYN_REFIT_N_MAX 4096
int mmdyn_plan_sample(const float* mean, const float* std, const float* eps, const float* keep, const float* lo, const float* hi,
                      float* cand, int N, int B, int T, int cd, void* stream);
int mmdyn_plan_refit(const float* cost, const float* cand, const float* mean_in, const float* std_in, float* mean_out,
                     float* std_out, uint8_t* elite, int* count, int K, int N, int B, int T, int cd, float alpha, float std_min,
                     void* stream);

/* ---- MPPI weights and the receding horizon (MVAEInference.plan_refine(temperature=..., warm_start=...)) --------------------
 * mmdyn_plan_refit_weighted: mmdyn_plan_refit with a weight on every elite.  Layouts, limits, the in-place allowance (mean_out /
 * std_out may be exactly mean_in / std_in) and the error codes are those of mmdyn_plan_refit.  Per row b:
 *   the ELITES are mmdyn_plan_refit's: the K smallest costs, ties to the lower n, a NaN never, +-Inf ordinary; K' their number.
 *   K == N cuts nothing, so nothing is ranked: n is an elite iff cost[n][b] is no NaN.
 *   c_min = the smallest elite cost.  In fp64, every operation rounded on its own (no fused multiply-add):
 *     w_n = 0 for a non-elite; w_n = 1, exactly, for an elite with cost_n == c_min (c_min = +-Inf included); otherwise
 *     w_n = exp(-(((double)cost_n - (double)c_min) / (double)temperature)) -- an elite at +Inf over a finite c_min: exp(-inf) = 0.
 *   W = sum w_n and Q = sum w_n * w_n in ascending n; ess[b] = (float)(W * W / Q), in [1, K'], and 0 when K' == 0.
 *   K' == 0: mean_out = mean_in, std_out = std_in, bit for bit.  Otherwise per element (t, d), over the candidates with
 *   w_n != 0 in ascending n (a candidate of weight zero is not loaded: its Inf / NaN reach nothing):
 *     m = (sum w_n * (double)c_n) / W;  v = (sum w_n * (((double)c_n - m) * ((double)c_n - m))) / W;  s = sqrt(v);
 *   then mmdyn_plan_refit's blend with alpha and its fmaxf(., std_min).  Equal elite costs make every weight 1 and W = K': the
 *   outputs then have the bits mmdyn_plan_refit writes.
 * weight (may be null): [N][B] double, w_n for every n, zeros included; ess (may be null): [B] float.  Neither may overlap any
 * other argument.  One block of 256 threads per row; LDS: mmdyn_plan_refit's 20 KB plus the fp64 weight column,
 * MMDYN_REFIT_N_MAX * 8 bytes = 32 KB (52 KB static).  No atomics, one fixed summation order: the same bits in every run.  The
 * only operation whose rounding the device's math library decides is exp (documented within 1 ulp).
 * Checked on the host: as mmdyn_plan_refit, and a weight that is not 8-byte aligned or weight / ess overlapping anything:
 * MMDYN_ERR_SHAPE; temperature not finite or not > 0: MMDYN_ERR_RANGE.
 *
 * mmdyn_plan_shift: the warm start of a horizon that has moved `shift` steps on, in one launch.  Every tensor [B][T][cd] fp32;
 * prev_keep and keep_out (the incumbent: the previous winner) are optional and come together.  For t + shift < T:
 *   mean_out[b][t] = prev_mean[b][t + shift];  keep_out[b][t] = prev_keep[b][t + shift];
 *   std_out[b][t] = fmaxf(prev_std[b][t + shift], widen * init_std[b][t]), the product one fp32 multiply (no fused operation);
 * for t + shift >= T (the tail): mean_out = keep_out = init_mean[b][t], std_out = init_std[b][t].  NaN and Inf are copied as
 * they are; fmaxf returns its other argument where one is a NaN (a NaN prev_std gives widen * init_std, a NaN product gives
 * prev_std) and a NaN where both are.  widen == 0 is the pure shift for non-negative std.  One element per thread, or 16-byte
 * accesses where cd % 4 == 0 and every pointer is 16-byte aligned (the same values either way).  No LDS, no atomics.
 * Checked on the host: prev_mean, prev_std, init_mean, init_std, mean_out or std_out null, or one of prev_keep / keep_out without
 * the other: MMDYN_ERR_NULL; B, T or cd < 1, shift outside [0, T], widen negative or not finite, or an output overlapping an
 * input or another output: MMDYN_ERR_SHAPE; B * T * cd >= 2^31: MMDYN_ERR_RANGE.
 * Both added without touching an existing signature or workspace: the revision stays 6. */
int mmdyn_plan_refit_weighted(const float* cost, const float* cand, const float* mean_in, const float* std_in, float* mean_out,
                              float* std_out, uint8_t* elite, int* count, double* weight, float* ess, int K, int N, int B, int T,
                              int cd, float temperature, float alpha, float std_min, void* stream);
int mmdyn_plan_shift(const float* prev_mean, const float* prev_std, const float* prev_keep, const float* init_mean,
                     const float* init_std, float* mean_out, float* std_out, float* keep_out, int B, int T, int cd, int shift,
                     float widen, void* stream);

/* ---- Adam (torch.optim.Adam defaults, problems.py:137-138) ----------------------------------- */
/* state: 3 doubles {step count, step size, sqrt(bias_correction2)}, advanced on the device by this call
 * (graph-replay safe); p/g/m/v: flat fp32 buffers of n elements; g is multiplied by grad_scale first */
int mmdyn_adam_step(float* p, const float* g, float* m, float* v, double* state, int64_t n, float lr,
                    float beta1, float beta2, float eps, float grad_scale, void* stream);
/* The same step behind an overflow guard (the fp16 precision modes: loss-scaled gradients can overflow fp16 on their way
 * through the matrix cores).  state: SIX doubles {step count, step size, sqrt(bias_correction2), flag, skipped steps, skip};
 * a gradient buffer that holds an inf or NaN leaves parameters, moments and step count untouched and adds one to state[4]
 * -- the behaviour of torch.cuda.amp.GradScaler.step on such a step (the reference itself trains in fp32: problems.py:150-155). */
int mmdyn_adam_step_guarded(float* p, const float* g, float* m, float* v, double* state, int64_t n, float lr,
                            float beta1, float beta2, float eps, float grad_scale, void* stream);

/* torch.optim.SGD with momentum / weight decay as configured by problems.py:132-136 (momentum 0.9, wd 5e-4);
 * first != 0 on the first step (momentum buffer := gradient, like torch) */
int mmdyn_sgd_step(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum,
                   float weight_decay, float grad_scale, int first, void* stream);

/* ---- clipping by the global L2 norm (torch.nn.utils.clip_grad_norm_), with the norm reported ---- */
/* clip: FOUR doubles on the device, owned by the caller and zeroed once: {S = sum of squares, norm, coefficient, clipped steps}.
 * Everything below runs on the device without a host read, so a captured step replays it.  Added without touching an existing
 * signature: the revision stays 6.
 *
 * mmdyn_grad_sumsq_blocks: host query, the number of fp64 partial sums a mmdyn_grad_sumsq over n elements writes (>= 1).  A
 * function of n alone (not of the device, not of an experiment variable), non-decreasing in n, at most 2048. */
int mmdyn_grad_sumsq_blocks(int64_t n);
/* clip[0] = sum_i g[i]^2 (accumulate != 0: clip[0] += ..., to chain the tensors of a parameter list), in two launches and without
 * float atomics: the result depends neither on arrival order nor on what `partials` held.  Block b of the first launch owns a fixed
 * contiguous chunk of g (its length follows from n alone); squares and sums are fp64 (an fp32 square is exact there); a thread
 * adds its 4-element groups in address order, then the 64-lane shuffle tree, the four wave totals in wave order, partials[b].  The
 * second launch is one block: thread t adds partials [t * per, (t + 1) * per), per = ceil(blocks / 256), in index order, then the
 * same tree.  Every partial it reads was written by the first launch of the same call.  Error against the exact sum: at most
 * 2 n 2^-53 relative.  g 16-byte aligned: 16-byte loads; g only 4-byte aligned (an offset view): dword loads of the same elements
 * in the same order, the same bits.  n == 0: S = 0 (unchanged when accumulating).
 * partials: mmdyn_grad_sumsq_blocks(n) doubles of workspace.
 * Checked on the host: partials or clip null, or g null with n != 0: MMDYN_ERR_NULL; n < 0 or g not 4-byte aligned:
 * MMDYN_ERR_SHAPE. */
int mmdyn_grad_sumsq(const float* g, int64_t n, double* partials, double* clip, int accumulate, void* stream);
/* One thread, fp64: clip[1] = norm = |grad_scale| sqrt(clip[0]); clip[2] = coef = min(1, max_norm / (norm + 1e-6)); clip[3] += 1
 * when coef < 1 and the norm is finite.  grad_scale: what the optimiser step multiplies the buffer by (1 / (world size * loss
 * scale)), so the norm is that of the gradient the step applies.  max_norm = +inf: coef is exactly 1 -- report, never clip.  A
 * non-finite S follows IEEE arithmetic (NaN -> norm and coef NaN; +inf -> norm inf, coef 0) and is never counted as clipped: what
 * such a step does is the guard's decision (mmdyn_adam_step_clipped).
 * Checked on the host: clip null: MMDYN_ERR_NULL; max_norm <= 0 or NaN: MMDYN_ERR_SHAPE. */
int mmdyn_grad_clip_coef(double* clip, float grad_scale, float max_norm, void* stream);
/* mmdyn_adam_step whose gradient factor is f = (float)((double)grad_scale * clip[2]) instead of grad_scale: with clip[2] == 1.0 the
 * step is mmdyn_adam_step's bit for bit, otherwise that of mmdyn_adam_step(grad_scale = f).  guarded != 0: state has SIX doubles
 * and the step is skipped and counted as mmdyn_adam_step_guarded does (state[4] += 1, nothing else moves) when clip[1], the norm,
 * is not finite -- a finite fp32 buffer cannot overflow the fp64 sum of its squares, so this is "the gradient holds inf / NaN"
 * without a second pass over it (state[3] is not used).  Unguarded, a non-finite norm goes through the arithmetic, as in torch.
 * Checked on the host: a null pointer: MMDYN_ERR_NULL. */
int mmdyn_adam_step_clipped(float* p, const float* g, float* m, float* v, double* state, const double* clip, int64_t n,
                            float lr, float beta1, float beta2, float eps, float grad_scale, int guarded, void* stream);
/* mmdyn_sgd_step with the same factor: d = g * f + weight_decay * p (the decay is added after the clipping, as in torch). */
int mmdyn_sgd_step_clipped(float* p, const float* g, float* momentum_buf, const double* clip, int64_t n, float lr,
                           float momentum, float weight_decay, float grad_scale, int first, void* stream);

/* ---- exponential moving average of the parameters (torch.optim.swa_utils.AveragedModel with an EMA rule, use_buffers=False) ---- */
/* ema_state: FOUR doubles on the device, owned by the caller: {updates done n, decay d, 1 - d_n of the current update, warm-up
 * flag}.  The caller writes d (in [0, 1)) and the flag once and zeroes the rest; everything below runs on the device without a host
 * read, so a captured step replays it.  Added without touching an existing signature: the revision stays 6.
 *
 * mmdyn_ema_tick: one thread, fp64.  d_n = d, or with the warm-up flag set min(d, (1 + n) / (10 + n)) for the count n BEFORE this
 * update; ema_state[2] = 1 - d_n, ema_state[0] = n + 1.  adam_state (nullable): the SIX-double state of a guarded Adam step whose
 * tick has already run; when its skip word (adam_state[5]) is set, the tick changes nothing -- a skipped step is no update of the
 * average.  Checked on the host: ema_state null: MMDYN_ERR_NULL. */
int mmdyn_ema_tick(double* ema_state, const double* adam_state, void* stream);
/* ema[i] = fmaf(omd, p[i] - ema[i], ema[i]) in fp32, omd = (float)ema_state[2]: the difference rounds once, the fused multiply-add
 * once.  One call per parameter tensor behind one mmdyn_ema_tick per optimiser step (the module path).  Both buffers 16-byte aligned:
 * 16-byte accesses and a scalar tail; otherwise (4-byte aligned views) dword accesses -- the same bits.  No atomics; no element
 * depends on the grid.  The call applies ema_state[2] as it stands: a caller whose step can be skipped uses mmdyn_adam_step_ema.
 * Checked on the host: ema_state null, or ema / p null with n != 0: MMDYN_ERR_NULL; n < 0, a buffer not 4-byte aligned, or ema
 * overlapping p: MMDYN_ERR_SHAPE. */
int mmdyn_ema_update(float* ema, const float* p, const double* ema_state, int64_t n, void* stream);
/* The Adam step that keeps the average in the same pass: p, g, m, v are read once, ema is read and written, each element of ema
 * moving towards the parameter value this step has just written, by the arithmetic of mmdyn_ema_update (same bits as the step
 * followed by mmdyn_ema_tick + mmdyn_ema_update).  clip null: mmdyn_adam_step (guarded == 0) or mmdyn_adam_step_guarded (guarded != 0)
 * bit for bit in p, m, v and state; clip non-null: mmdyn_adam_step_clipped(guarded).  One launch more than that step: the EMA tick,
 * behind Adam's.  A step the guard skips leaves ema and ema_state untouched as well.
 * Checked on the host: a null pointer other than clip: MMDYN_ERR_NULL; n < 0, ema not 16-byte aligned, or ema overlapping p:
 * MMDYN_ERR_SHAPE. */
int mmdyn_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, double* state, const double* clip,
                        double* ema_state, int64_t n, float lr, float beta1, float beta2, float eps, float grad_scale,
                        int guarded, void* stream);

/* ---- image grids of the epoch log (problems.py:580-604: torch.sigmoid, v[0][:n] / v[1][:n], torch.cat, ------------
 * torchvision.utils.make_grid(img, nrow) and the writer's float32 * 255 -> clip -> uint8) as ONE launch.
 * src0, src1 (nullable): contiguous fp32 [n_i][C][H][W], C in {1, 3}.  The image list is the first min(n0, take) images of src0
 * followed by the first min(n1, take) of src1 (torch.cat((v[0][:take], v[1][:take])); src1 null with n1 == 0 is the single-tensor
 * branch); N its length.  Layout = make_grid(img, nrow, padding, pad_value=0): xmaps = min(nrow, N), ymaps = ceil(N / xmaps),
 * Hg = ymaps * (H + padding) + padding, Wg = xmaps * (W + padding) + padding, image k at row (k / xmaps) * (H + padding) + padding
 * and column (k % xmaps) * (W + padding) + padding, every other pixel 0 (also the cells of a partly filled last row); C == 1 is
 * replicated to three channels; N == 1 is the image alone, Hg = H, Wg = W.
 * out: uint8 [Hg][Wg][3] (HWC, a PNG's scanlines), exactly Hg * Wg * 3 bytes: every byte of it is written (no memset in front), no
 * byte outside it is touched.  Value: v = logits ? 1 / (1 + exp(-x)) : x, t = v * 255.0f in fp32,
 * byte = t >= 255 ? 255 : (t > 0 ? (uint8)t : 0) -- truncation; NaN gives 0.  `logits` applies to both sources.
 * Added without touching an existing signature: the revision stays 6.
 * Checked on the host, before any launch: src0 or out null: MMDYN_ERR_NULL; src1 non-null with n1 <= 0, or null with n1 != 0; C not
 * 1 or 3; H, W, take, nrow or n0 below 1; padding < 0; a pointer not 4-byte aligned: MMDYN_ERR_SHAPE; Hg * Wg * 3 or a source's
 * element count >= 2^31: MMDYN_ERR_RANGE. */
int mmdyn_image_grid_u8(const float* src0, const float* src1, uint8_t* out, int n0, int n1, int take, int C, int H, int W,
                        int nrow, int padding, int logits, void* stream);

/* ---- image decode in front of the path --------------------------------------------------------
 * transforms.Resize(input_size) + transforms.ToTensor() of datasets.py:23-31 / 375-385 on frames kept as uint8
 * HWC in HBM: Pillow's 8-bit anti-aliased bilinear resampler (libImaging/Resample.c: 22-bit fixed-point taps,
 * horizontal then vertical pass, each rounded to uint8) followed by /255 -> float32 CHW.  Bit-exact.
 *   mmdyn_resize_ksize : taps per output sample for one axis (host only)
 *   mmdyn_resize_plan  : bounds[out][2] = (first tap, tap count), coeffs[out][ksize]; returns ksize (host only)
 *   mmdyn_resize_u8_to_chw_f32 : src uint8 [n][Hin][Win][3]; index (nullable) int32 [n_out] frame gather;
 *                        dst float32 [n_out][3][Hout][Wout]; xb/xk, yb/yk: the DEVICE copies of the two plans */
int mmdyn_resize_ksize(int in_size, int out_size);
int mmdyn_resize_plan(int in_size, int out_size, int* bounds, int* coeffs);
int mmdyn_resize_u8_to_chw_f32(const uint8_t* src, const int* index, float* dst, int n_out, int Hin, int Win,
                               int Hout, int Wout, const int* xb, const int* xk, const int* yb, const int* yk,
                               void* stream);

/* ---- bf16 activation storage (BASELINE configs[2]: "bf16 storage, fp32 accumulate / master weights") -----------
 * The activations between the convolution layers (pre-BatchNorm outputs, post-Swish activations and their
 * gradients) are bf16 in HBM (RNE on store, exact widening on load); weights, BatchNorm statistics and parameters,
 * the FC-level tensors, logits, losses and optimiser state stay fp32; all arithmetic is fp32 in registers except the
 * bf16 matrix-core products (fp32 accumulate).
 *   mmdyn_igemm_nt_mx : mmdyn_igemm_nt / _dgrad_bn with per-tensor storage flags --
 *       bit 0 bf16 matrix cores (required when any other bit is set), bit 1 A is bf16 (not IM2COL3), bit 2 C and
 *       C_act are bf16, bit 3 the BatchNorm-backward operand y is bf16, bit 4 the packed weights Bp are bf16
 *       (mmdyn_pack_conv_weight_b16 / mmdyn_repack2d_ld_b16 / a dst_bf16 plan entry), bit 6 C_act alone is bf16 (C stays
 *       fp32: the Linear layer whose activated output feeds the first transposed convolution, vae.py:264-271; not with
 *       bit 2 or split-K).  y == NULL: plain GEMM epilogue.  Split-K (fp32 workspace) is allowed with a bf16 A, not with a
 *       bf16 C.  Bit 5 together with bit 0: every tensor the other bits mark is IEEE HALF instead of bf16 and the product
 *       runs on the fp16 matrix cores (precision "fp16s": fp16 activation storage, BASELINE configs[4] arithmetic); bit 5
 *       with no storage bit is mmdyn_igemm_nt_f16.
 *       Bit 7 ALONE (flags == 128; also accepted by mmdyn_igemm_nt_dgrad_act / _grouped, mmdyn_wgrad_tn_mx / _grouped and the
 *       *_stat_tiles_mx / *_slab_floats_mx queries): an fp32 launch -- fp32 operands, fp32 results, every tensor fp32 in HBM --
 *       that MAY run on the bf16 matrix cores through the exact three-term split of its fp32 operands (precision "fp32x3" of the
 *       host side): x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid (round-to-nearest, both
 *       subtractions exact), six of the nine cross products (hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi) on
 *       v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the dropped products are below 2^-23 |a||b| together, less than one fp32
 *       rounding of the product, and the error against fp64 is no larger than the fp32 matrix cores' (csrc/common.h split3_bf16,
 *       csrc/igemm_nt.hip / wgrad_tn.hip X3; profiles/r4/ab_x3_*.txt).  The library decides per launch (shapes with >= 512 blocks
 *       of 64x64 or >= 384 of 128x128 outputs; every weight-gradient GEMM); the rest of such a step runs the fp32 matrix cores.
 *       Operand range (tests/test_kernels_aten_gpu.py::test_x3_operand_magnitudes_*, ::test_x3_non_finite_*): full fp32 accuracy
 *       for 2^-100 <= |x| < 0x1.ffp+127 (bit pattern 0x7F7F8000, ~3.39e38: from there to FLT_MAX bf16's round-to-nearest takes the
 *       high term to Inf and the split gives NaN, like an Inf operand).  Below 2^-100 the lower terms of the split leave bf16's normal range and are flushed by the matrix
 *       pipe: an operand under ~1e-33 keeps 16 significant bits, one under ~3e-36 keeps 8 -- an absolute error of at most
 *       2^-126 |w| per product.  An Inf operand gives NaN (inf - inf in the split) where the fp32 matrix cores would give Inf; a
 *       NaN operand gives NaN; no other row of the result is touched.  The library does not guard: non-finite operands do not occur
 *       on this path (the fp16 modes' overflow guard, mmdyn_adam_step_guarded, is not needed in fp32 storage).
 *       Bit 10 (with bits 7 + 8, DENSE launches; round 6): C_act is written as a plane tensor -- the activated output of a Linear
 *       layer handed to the next plane launch without a stand-alone split; C stays fp32, ldc == N.  Bits 16-27 = c / 8: the plane
 *       rows hold c channels, c dividing N (an output row is N / c consecutive plane rows: the decoder's Linear output
 *       [B][hw*256 + ch] read as [B*25][256] by the transposed convolution above it, vae.py:264-271); 0: rows of [plane][N].
 *       Bits 7 + 8 (flags == 384; mmdyn_igemm_nt_mx, mmdyn_igemm_nt_dgrad_act; mmdyn_igemm_nt_dgrad_bn(bf16 = 4)): the same
 *       arithmetic on operands that ARRIVE SPLIT -- A and Bp are rows of [plane][Cin] bf16 (hi | mid | lo, 6 bytes per element:
 *       mmdyn_split_planes, or written so by their producers) -- so the GEMM itself contains no split: LDS-DMA of the planes, six
 *       v_mfma_f32_16x16x32_bf16 per fragment pair (csrc/igemm_wsp.hip, igemm_wsp3_kernel; the 32-channel up-sampling layers:
 *       csrc/tconv_patch.hip, tconv_patch_kernel<..., P3>).  Same terms, same product order per
 *       K-step as the flags == 128 launch of the shape (results agree to the last bits; the channel -> k-lane map inside the 32-deep
 *       MFMA differs, so not bit for bit).  Only for shapes mmdyn_igemm_planes_served answers 1 for
 *       (MMDYN_ERR_SHAPE otherwise); partial-sum tile count and workspace: the *_stat_tiles_mx / *_slab_floats_mx queries with flags == 384.
 *   mmdyn_wgrad_tn_mx : bit 0 as above, bit 1 D is 16-bit, bit 2 Gt is 16-bit (not IM2COL3), bit 5 as above, bit 7 alone as above;
 *       with bit 7, bit 8: D arrives split, bit 9: Gt arrives split (plane tensors, rows of [plane][C] bf16; MMDYN_CONV only) -- that
 *       operand goes from HBM to the LDS planes as it is, the other is split in the kernel as with bit 7 alone; both bits: the
 *       plane-ring weight-gradient kernel where it serves the channel counts (csrc/wgrad_p3.hip; chunks from mmdyn_wgrad_chunks_mx
 *       with the same flags).
 *   *_b16             : the element-wise kernels on 16-bit activation tensors (half = 0: bf16, half = 1: IEEE half). */
int mmdyn_igemm_nt_mx(const void* A, const void* Bp, const float* bias, void* C, void* C_act, float* stats,
                      float* ws, const void* y, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N,
                      int ldc, int stride, int offset, int act, int splitk, int flags, uint32_t* arrival_flags, void* stream);
int mmdyn_wgrad_tn_mx(const void* D, const void* Gt, float* partial, int mode, int Bt, int Hr, int Wr, int Cd, int Hi,
                      int Wi, int Cg, int stride, int offset, int chunks, int flags, void* stream);
/* The exact three-term bf16 split of an fp32 matrix, stored for the plane launches above: x [rows][C] fp32 ->
 * planes [rows][3][C] bf16 with planes[r][0] = hi = bf16(x), [1] = mid = bf16(x - hi), [2] = lo = x - hi - mid (round-to-nearest-
 * even; hi + mid + lo == x bit for bit for finite x).  C % 8 == 0.  A channels-last activation tensor is such a matrix with one
 * row per pixel; packed weights [taps][N][Cin] are one with taps * N rows.  (Replaces nothing in the reference: it is the storage
 * format of the fp32x3 arithmetic's GEMM operands, the role nn.Conv2d's fp32 input tensor plays in vae.py:198-216, 264-277.) */
int mmdyn_split_planes(const float* x, void* planes, int64_t rows, int C, void* stream);
int mmdyn_igemm_planes_served(int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N);
/* mmdyn_bn_swish_fwd / mmdyn_bn_swish_bwd_apply (train-mode nn.BatchNorm2d + Swish forward, vae.py:200-208, 268-276, and the apply
 * pass of their backward) with the result ALSO (a / dy non-null) or ONLY (a / dy NULL) written as a plane tensor -- the split
 * rides on a pass that exists anyway, so the GEMMs that consume the tensor find their operand already split. */
int mmdyn_bn_swish_fwd_planes(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                              float* a, void* a_planes, int G, int rows_per_group, int C, void* stream);
int mmdyn_bn_swish_bwd_apply_planes(const float* da, const float* y, const float* mean, const float* rstd, const float* gamma,
                                    const float* beta, const float* sums, float* dy, void* dy_planes, int G, int rows_per_group,
                                    int C, int da_is_du, void* stream);
/* The 3-channel layers' direct kernel (csrc/conv3.hip) with plane-row outputs, for the fp32x3 arithmetic on fp32 storage: the
 * 32-channel tensor the kernel produces goes to HBM as the plane tensor its consumer GEMMs take ([rows][3][32] bf16, the exact
 * three-term split as mmdyn_split_planes writes it, bit for bit), so no fp32 copy of it and no stand-alone split pass exist.
 * Images are [G * Bg][3][H][H] fp32 NCHW with H = 64 (any other H: MMDYN_ERR_SHAPE), Wp the packed [32][64] fp32 weight of
 * mmdyn_igemm_nt's MMDYN_IM2COL3 mode, rows = G * Bg * (H/2)^2.  Null pointer: MMDYN_ERR_NULL; rows * 32 >= 2^31: MMDYN_ERR_RANGE;
 * both before anything is launched.
 *   mmdyn_conv3_fwd_planes: Conv2d(3, 32, 4, 2, 1) forward (vae.py:198).  C [rows][32] fp32 = the pre-activation, exactly
 *     mmdyn_igemm_nt(MMDYN_IM2COL3)'s C; act_planes = the split of act(C), exactly mmdyn_split_planes of that launch's C_act
 *     (act: MMDYN_ACT_NONE / SWISH / RELU, anything else MMDYN_ERR_SHAPE).
 *   Input gradient of ConvTranspose2d(32, 3, 4, 2, 1) (vae.py:277) through the train-mode BatchNorm + Swish below it, in two
 *   passes of one main loop instead of mmdyn_igemm_nt_dgrad_bn + mmdyn_bn_swish_bwd_apply_planes(da_is_du = 1) -- du, which
 *   existed only to cross the finalize between them, is recomputed by the second pass and never stored:
 *   mmdyn_conv3_dgrad_bn_stats: stats [G][T][2][32], T = mmdyn_igemm_stat_tiles(MMDYN_IM2COL3, ...): the per-tile sums of du and
 *     du * xhat, the table mmdyn_igemm_nt_dgrad_bn writes for the same inputs, bit for bit;
 *   mmdyn_conv3_dgrad_bn_apply_planes: sums [G][2][32] = the finalized sums (mmdyn_bn_bwd_finalize / _finalize_sums);
 *     dy_planes = dL/dy as plane rows, the bits mmdyn_bn_swish_bwd_apply_planes(da_is_du = 1) writes from the stored du.
 * Added without touching an existing signature or workspace: the revision stays 6. */
int mmdyn_conv3_fwd_planes(const float* x, const float* Wp, float* C, void* act_planes, int G, int Bg, int H, int act,
                           void* stream);
int mmdyn_conv3_dgrad_bn_stats(const float* dlogits, const float* Wp, float* stats, const float* y, const float* mean,
                               const float* rstd, const float* gamma, const float* beta, int G, int Bg, int H, void* stream);
int mmdyn_conv3_dgrad_bn_apply_planes(const float* dlogits, const float* Wp, const float* y, const float* mean,
                                      const float* rstd, const float* gamma, const float* beta, const float* sums,
                                      void* dy_planes, int G, int Bg, int H, void* stream);
/* Backward of EVAL-mode nn.BatchNorm2d + Swish (vae.py:200-208, 268-276 under module.eval(): F.batch_norm(training=False), whose
 * autograd the reference gets for free) in ONE pass over [G * rows_per_group][C], fp32, shapes as the kernels above.  The forward
 * is u = gamma * (y - mean) * rstd + beta, a = swish(u), with mean / rstd [G][C] the running estimates (mmdyn_bn_eval_stats):
 * constants, so there are no batch-mean terms:  du = da_is_du ? da : da * swish'(u),  dy = du * gamma * rstd.
 *   dy (fp32) and / or dy_planes (the plane tensor of mmdyn_bn_swish_bwd_apply_planes): at least one is required;
 *   partial (nullable) [G][T][2][C], T = mmdyn_colstats_tiles(rows_per_group): per tile sum du and sum du * xhat -- the layout and
 *   meaning of mmdyn_bn_swish_bwd_reduce's output, so mmdyn_bn_bwd_finalize turns it into dgamma / dbeta; written by the same pass
 *   from the values in registers, in a fixed order (no atomics);
 *   with da_is_du = 1 and partial == NULL neither u nor xhat is needed: y is not read and may be NULL.
 * Added without touching an existing signature or workspace: the revision stays 6. */
int mmdyn_bn_eval_swish_bwd(const float* da, const float* y, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, float* dy, void* dy_planes, float* partial, int G, int rows_per_group, int C,
                            int da_is_du, void* stream);
int mmdyn_bn_swish_fwd_b16(const uint16_t* y, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, uint16_t* a, int G, int rows_per_group, int C, int half, void* stream);
int mmdyn_bn_swish_bwd_reduce_b16(const uint16_t* da, const uint16_t* y, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, float* partial, int G, int rows_per_group,
                                  int C, int half, void* stream);
int mmdyn_bn_swish_bwd_apply_b16(const uint16_t* da, const uint16_t* y, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const float* sums, uint16_t* dy, int G,
                                 int rows_per_group, int C, int da_is_du, int half, void* stream);
int mmdyn_act_bwd_b16(const uint16_t* dh, const uint16_t* u, uint16_t* du, int64_t n, int act, int half, void* stream);
int mmdyn_tconv_out3_fwd_b16(const uint16_t* a, const float* w, float* out, int Bt, int Hi, int Wi, int half,
                             void* stream);

/* ---- misc ------------------------------------------------------------------------------------- */
int mmdyn_nchw_to_nhwc(const float* in, float* out, int B, int C, int HW, void* stream);
int mmdyn_nhwc_to_nchw(const float* in, float* out, int B, int C, int HW, void* stream);

/* ---- conditional models: the operand join ------------------------------------------------------
 * out [rows][width] = [x | condition | 0]: out[r][0:K) = x[r][0:K) (x has its own row stride ldx >= K), out[r][K:K+cd) = the
 * condition of row r, out[r][K+cd:width) = 0.  width % 32 == 0 (the K-step of the GEMM that consumes out), K + cd <= width.
 * Exactly one condition source is non-null (MMDYN_ERR_NULL otherwise):
 *   cond     [rows][cd] fp32 : real-valued conditions -- torch.cat((x, c.float()), dim=-1), vae.py:231-237 (encoder heads) and
 *                              vae.py:286-291 (decoder input);
 *   cond_idx [rows] int64    : categorical conditions -- the one-hot row of idx2onehot (vae.py:337-344: the assert, the
 *                              torch.zeros and the scatter_) is written by the kernel; no one-hot tensor exists in memory.
 * An index outside [0, cd) is input, not a fault: that row's condition block is all zero and bit 0 of *bad_index (nullable) is
 * OR-ed in; the caller clears the word and reads it where it synchronises anyway (the reference asserts with a host read-back,
 * vae.py:338).  Every element of out is written, the padding included.  Pure copy: bit-identical to torch.cat + zero padding.
 * One launch (16-byte accesses when K % 4 == 0, ldx % 4 == 0 and x / out are 16-byte aligned, one element per thread otherwise);
 * replaces the memset + two mmdyn_repack2d_ld launches per consumer. */
int mmdyn_concat_condition(const float* x, const float* cond, const int64_t* cond_idx, float* out, int* bad_index, int rows,
                           int K, int ldx, int cd, int width, void* stream);
/* The tiled join: x holds x_rows rows and out row r reads x[r % x_rows]; cond / cond_idx, out and bad_index keep one entry per out
 * row, exactly as above.  The operand [h[r mod B] | candidate of row r | 0] of N candidate conditions per row of a batch, written
 * without the features being repeated in memory.  rows % x_rows != 0 (or x_rows < 1): MMDYN_ERR_SHAPE; the range check covers
 * x_rows * ldx.  The same kernels as mmdyn_concat_condition, which is this call with x_rows == rows: every property above holds
 * (both access paths, every element of out written, the one-hot written by the kernel, a bad index served as zeros and reported).
 * Added without touching an existing signature or workspace: the revision stays 6. */
int mmdyn_concat_condition_tiled(const float* x, const float* cond, const int64_t* cond_idx, float* out, int* bad_index, int rows,
                                 int x_rows, int K, int ldx, int cd, int width, void* stream);

#ifdef __cplusplus
}
#endif
#endif
