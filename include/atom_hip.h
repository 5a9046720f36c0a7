/*
 * atom_hip.h -- C ABI of libatom_hip.so: MI355X (gfx950) implementation of Atom's W4A4
 * mixed-precision GEMM hot path.
 *
 * Every entry point replaces one host launcher of the reference (file:line relative to
 * /root/reference).  Conventions, all entry points:
 *   - plain device pointers + sizes, no framework types; caller owns every buffer; nothing is
 *     allocated, nothing is synchronised; the launch is enqueued on `stream` (a hipStream_t passed
 *     as void*; NULL = the null stream).  Re-entrant and thread-safe (no global state).
 *   - returns ATOM_OK (0) or a negative ATOM_ERR_* code; shapes/alignment are validated BEFORE any
 *     launch (the reference validates nothing: e2e/punica-atom/punica/ops/csrc/punica_ops.cc:73-80,
 *     211-262).  atom_strerror() names a code.
 *   - group size 128 and keeper (INT8 outlier columns) 128 are the only supported values, as in the
 *     reference (GROUP_SIZE/KEEPER macros, kernels/include/GEMM/Dense_layer_gemm_i4_o16.cuh:35,54).
 *
 * Data formats (identical to the reference unless noted):
 *   A4 / B4   uint8 [rows, K4/2]   two's-complement int4, element 2j in the LOW nibble, 2j+1 in the
 *                                   HIGH nibble (PackInt4, kernels/include/Reorder/Reorder.cuh:16-19)
 *   A8 / B8   int8  [rows, 128]    keeper columns (the LAST 128 reordered channels)
 *   sB        fp16  [G, N]         weight scales, G = K4/128 (Dense_layer_gemm_i4_o16.cuh:497)
 *   sB8       fp16  [N]
 *   sA, sA8   fp16  activation scales, one of two layouts selected by `scale_layout`:
 *       ATOM_SCALE_LAYOUT_REF   (0): the reference's ldmatrix-replicated layout -- row r of group g
 *                                    at g*atom_scale_size(M,0) + scale_index(r) + 2j, j=0..3
 *                                    (Reorder.cuh:39-50,137-156)
 *       ATOM_SCALE_LAYOUT_PLAIN (1): [G, M] row-major (sA8: [M]); the native layout.
 *   K_total = K4 + 128 (the e2e convention, e2e/.../GEMM/DenseLayerGEMM_i4.cu:764).
 */
#ifndef ATOM_HIP_H_
#define ATOM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATOM_OK 0
#define ATOM_ERR_INVALID_ARG (-22)  /* null pointer, bad enum */
#define ATOM_ERR_SHAPE (-33)        /* unsupported M/N/K/hidden/group/keeper */
#define ATOM_ERR_ALIGN (-14)        /* pointer not 16-byte aligned */
#define ATOM_ERR_LAUNCH (-5)        /* hipGetLastError() != hipSuccess after the launch */

#define ATOM_SCALE_LAYOUT_REF 0
#define ATOM_SCALE_LAYOUT_PLAIN 1

/* Quantisation arithmetic of the three activation ops */
#define ATOM_QUANT_KERNEL 0 /* the reference CUDA kernels: FP32, q = round_half_away(x*(1/s)), s = amax*clip/qmax
                               (Reorder.cuh:137-178).  clip = 1.0 reproduces them exactly. */
#define ATOM_QUANT_SIM 1    /* the reference simulated path: FP16 opmath, amax.clamp(1e-5)*clip, q = rint(x/s)
                               (model/quant.py:141-142,166-172,181).  clip = args.a_clip_ratio. */

/*
 * Native activation format (no reference counterpart): OR ATOM_QUANT_WIDE_CODES into `quant_mode` of the three
 * activation ops and ATOM_A_WIDE into `scale_layout` of atom_gemm_w4a4_f16 / _ws.  o_norms / A4 is then
 *   int8 [M, K4]   byte[m, 32c + 16p + j] = 16 * code[m, 32c + 2j + p]   (c = 32-channel block, p = parity, j < 16)
 * i.e. the INT4 codes already widened to the INT8 MFMA operand (x16, the factor 1/256 is folded into the scales as for
 * packed operands) with the even / odd channels of every 32-channel block de-interleaved -- exactly the two operands the
 * GEMM otherwise makes from one packed 16-byte chunk with 3 VALU instructions per MFMA.  Costs K4/2 more bytes per
 * token in HBM, transient.  Same results bit for bit.  Not accepted by atom_gemm_w4a4_o4; always runs the tile
 * kernels (use the packed format for decode batches, M <= 256: they have their own kernels).
 */
#define ATOM_QUANT_WIDE_CODES 0x100
#define ATOM_A_WIDE 0x100

/*
 * Native "F6" operand format of the block-scaled-MFMA prefill kernel (gemm_w4a4_f6.hip; no reference counterpart): every
 * INT4 code is a BF6 (E3M2) number, and v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4 with unit block scales multiply them exactly
 * at the FP4 rate.  OR ATOM_AB_F6 into `scale_layout` of atom_gemm_w4a4_f16: BOTH A4 and B4 are then
 *   uint8 [G][atom_f6_rows(rows)][104]   group-major; bytes 0..95 = the 128 codes of (row, group) as a little-endian
 *                                         stream of 6-bit BF6 fields; A4 only: bytes 96..97 = the fp16 scale of (row,
 *                                         group), 98..99 zero, 100..103 = the same scale as fp32 (the GEMM reads token
 *                                         scales from the row, `sA` is ignored); B4: bytes 96..103 zero
 * with atom_f6_rows(rows) = rows rounded up to 256 (pad rows: any bytes).  sB / keeper operands and scales as before.  OR
 * ATOM_B_F6S in as well when the B4 buffer is followed by the weight scales as float32 [G][atom_f6_rows(N)] (pad columns
 * zero; atom_repack_weight_f6s writes both, offline with the weight): the 256x256 kernel then streams them straight into its
 * de-quantisation registers (no fp16 -> fp32 conversions in the K loop); `sB` (fp16) is still required -- the other tile
 * geometries read it.
 * Activations: ATOM_QUANT_F6_CODES in `quant_mode` of the three activation ops (o_norms = that buffer; norm_scales is
 * still written).  Weights: atom_repack_weight_f6 / atom_repack_weight_f6s.  M, N >= 1 as usual; tile geometries picked by shape, all
 * with the K steps summed in order -- results bit-identical to the INT8 kernels --: 64x64 / 128x64 tiles over the whole K range on a
 * deep LDS ring while a shape has at most 512 tiles of 64x64 (round 5: 256x4096x4096 11.0 us, 512x4096x4096 14.7), 256x256 where
 * those fill the chip (4096^3: 48.5-50 us), 256x128 and 128x128 (4 waves) between -- EXCEPT shapes beyond 512 tiles of 64x64 with at
 * most 256 tiles of 128x128 (and >= 8 K steps; 1024x4096x4096: 23 us): their 128x128 tiles are shared by two groups of 4 waves that
 * split the G + 1 K steps (the G int4 groups, then the keeper) at (G + 1) / 2: each half is summed in order from 0 and
 * D = half(first + second) -- deterministic, same tolerance.  atom_gemm_w4a4_f6_order(M, N, K_total) tells which: 1 = K steps in
 * order, 2 = two halves (4 = four ranges: tuning builds only; 0 = unsupported shape).
 * Ahead of the INT8 kernels from 129 rows up (1.7x at 512-1024 rows, 1.8x at 4096^3).
 */
#define ATOM_QUANT_F6_CODES 0x200
#define ATOM_AB_F6 0x200
int atom_gemm_w4a4_f6_order(int64_t M, int64_t N, int64_t K_total);
#define ATOM_B_F6S 0x400
/* atom_gemm_w4a4_o4 / _o4_ws only: the u4 epilogue exactly as the reference CODE computes it -- its local_max_min takes abs() of
 * both extrema (DenseLayerGEMM_i4_o4.cu:73-80), so scale = (max|x| - min|x|) / 15, zero = -min|x|, and the code is
 * (int8)round((x + zero) / scale) & 0xF (no clamp: negative results wrap, :766-771).  Wrong for any group with negative values
 * (its consumer de-quantises code * scale - zero, flashinfer/quantization.cuh:59-84); the default implements the intended
 * min / max.  Opt-in, for bit-comparisons against a reference run. */
#define ATOM_O4_REF_EXTREMA 0x800
/* atom_gemm_w4a4_f16_ws with PACKED operands on its re-coding route (use (2) below) only: the weight region of `workspace` already
 * holds the F6 form of exactly these B4 / sB (N, K_total) -- written by an earlier call with the same workspace and weight (the
 * weight of a layer is static) -- so only the activation is re-coded: 5 instead of 10 us of re-coding at 4096^3.  The library keeps no
 * state: the CALLER asserts it (atom_amd.ops tracks which weight its workspace holds).  Wrong flag = wrong results, never a fault
 * (the region is inside the workspace either way).  Ignored on every other route.
 * Round 5: with the flag the re-coding route starts at 129 rows (N >= 2048, K >= 1024; at 17 rows where the decode-batch kernel does
 * not take the shape: atom_gemm_w4a4_ws_recodes_cached) -- only the activation is re-coded, and the mid-size-batch kernel behind it runs
 * 129 .. 256 rows in ~11 us at 4096 x 4096 where the decode-batch kernel takes 9.4 .. 15.5, 64 x 13824 x 5120 in 12 us --, so a
 * caller that keeps ONE workspace per weight (a layer's weight is static) fills its weight region once, offline, with
 * atom_repack_weight_f6s(B4, sB, N, K_total, workspace, stream) -- the region's layout is exactly that function's output -- and passes
 * the flag on every call; atom_gemm_w4a4_workspace_bytes() covers those shapes, atom_gemm_w4a4_packed_order(.., 2) names their order. */
#define ATOM_WS_WEIGHT_CACHED 0x1000
/* OR into `scale_layout` of the GEMM entry points: the caller asserts that output channels 2 j and 2 j + 1 share their weight scales,
 * sB[g][2 j] == sB[g][2 j + 1] for every group g (weight_channel_group = 2 of model/qLinearLayer.py:63-70 -- the only form the
 * reference kernel accepts: its dequant applies ONE scale product to both columns of a pair, Dense_layer_gemm_i4_o16.cuh:413-431).
 * The 256x256 block-scaled-MFMA kernel then forms each (token, channel pair, group) scale product once: 6 instead of 8 de-quantisation
 * instructions per MFMA.  Same results bit for bit when the assertion holds; channel 2 j + 1 is de-quantised with channel 2 j's scale
 * when it does not (never a fault).  sB8 -- the keeper's scales are per output channel, model/qLinearLayer.py:59 -- is not covered:
 * the keeper step always forms one product per channel.  Ignored by kernels that do not use it. */
#define ATOM_B_SCALE_PAIRS 0x2000
/* atom_gemm_w4a4_f16_ws only, DEBUG: verify the two assertions above on the device before relying on them -- ATOM_B_SCALE_PAIRS against
 * the values of sB (packed operands), ATOM_WS_WEIGHT_CACHED by re-coding B4 / sB and comparing with the workspace's weight region --
 * and return ATOM_ERR_INVALID_ARG instead of computing wrong numbers when one does not hold.  Needs a workspace of
 * atom_gemm_w4a4_workspace_bytes() (its last 16 bytes serve as the counter before the GEMM uses them); SYNCHRONISES the stream (the one
 * exception to "no synchronisation" in this ABI), so it is not for production calls nor for graph capture.  The reference guards
 * its KV ops the same way at the binding (TORCH_CHECK in punica_ops.cc:18-47); a binding without a debug mode asks the two functions
 * below once per weight instead. */
#define ATOM_WS_VERIFY 0x4000
#define ATOM_F6_PITCH 104

const char *atom_version(void);
const char *atom_strerror(int code);

/* == python scale_size() for layout 0 (punica/ops/__init__.py:137-138, SCALE_SIZE_A Reorder.cuh:50);
 * == rows for layout 1.  Unit: halves. */
size_t atom_scale_size(int64_t rows, int scale_layout);

/*
 * D[M,N] (fp16) = sum_g (A4_g . B4_g^T) * sA[m,g] * sB[g,n]  +  (A8 . B8^T) * sA8[m] * sB8[n]
 * Replaces: DenseLayerGEMM_i4_o16 (kernels/include/GEMM/Dense_layer_gemm_i4_o16.cuh:728-769) and
 *           DenseLayerGEMM_i4<nv_half> (e2e/punica-atom/punica/ops/csrc/GEMM/DenseLayerGEMM_i4.cu:722-791).
 * Integer dot products are exact (INT8 / BF6 MFMA); per group s = sA[m,g] * sB[g,n] -- EXACT in FP32: both are fp16 values, 11-bit
 * significands -- and c = fma(idot, s, c): one rounding per group, groups in order, then the keeper: ONE dot product over its 128
 * columns, de-quantised once the same way -- the reference kernel accumulates both keeper k-steps in int32 before its dequant too
 * (Dense_layer_gemm_i4_o16.cuh:640-691); D = half(c).  This is the reference kernel's own dequant shape -- scale product first
 * (__hmul2, :417), then accu += c_frag * rs_scale (:419-431) -- without its two extra roundings (the FP16 product, the FP32 multiply
 * ahead of the add).  (Rounds 1-4 of this library: t = round_f32(idot * sA), c = fma(t, sB, c).)  The decode kernels
 * (M = 1: dot products along K; 2 <= M <= 256 in the packed format: eight waves own an eighth of the groups each) apply
 * the same per-group arithmetic and add their per-lane / per-wave partial sums in a fixed order: deterministic, within
 * 1 fp16 ulp of the exact value like the tile kernels, but not the same FP32 summation order.
 * Constraints: (K_total-128) % 128 == 0, K_total >= 256, N % 64 == 0, M >= 1, all pointers 16-byte aligned.
 */
int atom_gemm_w4a4_f16(const void *A4, const void *B4, const void *sA, const void *sB,
                       const void *A8, const void *B8, const void *sA8, const void *sB8,
                       void *D, int64_t M, int64_t N, int64_t K_total,
                       int group, int keeper, int scale_layout, void *stream);

/*
 * Same result, with an optional caller-owned scratch buffer.  Two uses: (1) skinny shapes (few output tiles) split
 * the K loop over several workgroups: FP32 partial sums [splits, M, N] are written to `workspace` and reduced, in split
 * order, by a second launch on the same stream; (2) PACKED operands of prefill size (M > 256 -- or > 128 where the decode-batch kernel does not take the shape --,
 * N >= 2048, K >= 1024) are re-coded into the F6 format inside the workspace (one bandwidth-bound launch; the activation alone
 * with ATOM_WS_WEIGHT_CACHED) and multiplied by the BF6-MFMA kernels: 55-60 instead of 89 us at 4096^3, 17.5 (weight cached;
 * 24.3 not) at 512x4096x4096, 26.2 (33.4) at 1024x4096x4096 (round 5); bit-identical to atom_gemm_w4a4_f16 where
 * atom_gemm_w4a4_f6_order(M, N, K_total) == 1, the sum of two / four ordered ranges of the K steps where it is 2 / 4 (see ATOM_AB_F6).
 * atom_gemm_w4a4_workspace_bytes() returns the size that enables it
 * (0 = the shape does not benefit; then, or with a NULL / too small workspace, this is atom_gemm_w4a4_f16).
 * The reference has no counterpart (its 128x128 tile kernel runs every M, bench_dense_layer_gemm_i4_o16.cu:64-69).
 * FP32 summation order differs from the unsplit kernel (per-split partial sums, then their sum): same tolerance.
 */
size_t atom_gemm_w4a4_workspace_bytes(int64_t M, int64_t N, int64_t K_total);
/* 1 when atom_gemm_w4a4_f16_ws takes use (2) for packed operands of this shape (the workspace then starts with the re-coded weight:
 * F6 records + float32 scales, atom_f6_weight_bytes(N, K_total) bytes, whatever M is -- what ATOM_WS_WEIGHT_CACHED refers to) */
int atom_gemm_w4a4_ws_recodes(int64_t M, int64_t N, int64_t K_total);
/* ... the same question for a call that passes ATOM_WS_WEIGHT_CACHED (the weight region holds this weight's BF6 form already, only the
 * activation is re-coded): additionally every shape of 129 rows and more, and from 17 rows the shapes the decode-batch kernel does not
 * take (N >= 2048, K >= 1024 throughout).  What a binding that keeps one workspace per weight asks. */
int atom_gemm_w4a4_ws_recodes_cached(int64_t M, int64_t N, int64_t K_total);
/* Checkers of the caller assertions (asynchronous on `stream`, no synchronisation; the count is a device int32 the caller reads):
 *   atom_check_scale_pairs   *n_bad_dev = number of (group, channel pair) of sB fp16 [G][N] whose two scales differ -- 0 means
 *                            ATOM_B_SCALE_PAIRS may be asserted for this weight (what atom_amd/ops.py:scale_pairs_shared computes in torch)
 *   atom_verify_weight_f6s   *n_bad_dev = number of (row < N, group) whose F6 record or float32 scale in B_f6s (atom_f6_weight_bytes(N,
 *                            K_total) bytes: a workspace's weight region) is not what atom_repack_weight_f6s makes of B4 / sB -- 0 means
 *                            ATOM_WS_WEIGHT_CACHED may be asserted for this (workspace, weight)
 * No reference counterpart (its launcher has neither flag; its bindings check what they can with TORCH_CHECK, punica_ops.cc:18-47). */
int atom_check_scale_pairs(const void *sB, int64_t G, int64_t N, int32_t *n_bad_dev, void *stream);
int atom_verify_weight_f6s(const void *B4, const void *sB, int64_t N, int64_t K_total, const void *B_f6s, int32_t *n_bad_dev, void *stream);
int atom_gemm_w4a4_f16_ws(const void *A4, const void *B4, const void *sA, const void *sB,
                          const void *A8, const void *B8, const void *sA8, const void *sB8,
                          void *D, int64_t M, int64_t N, int64_t K_total,
                          int group, int keeper, int scale_layout,
                          void *workspace, size_t workspace_bytes, void *stream);
/* The FP32 summation order atom_gemm_w4a4_f16 (with_workspace = 0) / atom_gemm_w4a4_f16_ws with a workspace of
 * atom_gemm_w4a4_workspace_bytes() bytes (with_workspace = 1) applies to PACKED (reference-format) operands of this shape -- a host-side
 * function of the shape alone, what the parity tests restate the arithmetic for (oracle/atom_oracle.c):
 *   1        the K steps (int4 groups, then the keeper) in order: the tile kernels -- among them the mid-size-batch kernels
 *            (gemm_w4a4_mid.hip: 64 x 64 / 128 x 64 tiles on a deep LDS ring; the INT8 form for 17 .. 256 rows with 96 .. 256 tiles, the
 *            BF6 form behind the re-coding routes up to 512 tiles of 64 x 64)
 *   2        two ordered ranges of the K steps (the BF6 two-wave-group kernel behind the re-coding routes; see ATOM_AB_F6)
 *   8        the decode-batch kernel: the G + 1 steps dealt to 8 waves in consecutive slices, partial sums added in wave order
 *   64       the one- / two-token dot-product kernel: groups dealt to 16 quad leaders, 64-lane butterfly, keeper last
 *   63       the staged dot-product kernel (M <= 7 with a K too long for the decode-batch kernel): per-lane partial sums
 *   100 + s  split-K over s workgroups through the workspace, partial sums added in split order
 *   0        unsupported shape
 * with_workspace = 2: a workspace AND ATOM_WS_WEIGHT_CACHED (the re-coding route from 129 rows, and from 17 rows for the shapes the
 * decode-batch kernel does not take: atom_gemm_w4a4_ws_recodes_cached). */
int atom_gemm_w4a4_packed_order(int64_t M, int64_t N, int64_t K_total, int with_workspace);

/*
 * Same GEMM; epilogue asymmetric-quantises every 128-wide output group to u4:
 *   scale = (max-min)/15, zero = -min, q = round((x+zero)/scale) & 0xF
 * D_u4 uint8 [M, N/2] (same nibble order), D_scale_zero fp16 [M, N/128, 2] = (scale, zero).
 * Replaces: DenseLayerGEMM_i4_o4 (e2e/.../GEMM/DenseLayerGEMM_i4_o4.cu:808-856, epilogue :704-788).
 * Constraint in addition: N % 128 == 0.
 */
int atom_gemm_w4a4_o4(const void *A4, const void *B4, const void *sA, const void *sB,
                      const void *A8, const void *B8, const void *sA8, const void *sB8,
                      void *D_u4, void *D_scale_zero, int64_t M, int64_t N, int64_t K_total,
                      int group, int keeper, int scale_layout, void *stream);

/*
 * Decode batches: ONE launch for the projections of a decode step that share an activation operand (no reference counterpart: the
 * reference launches dense_layer_gemm_i4_fp16 / _o4 once per projection, punica/models/llama.py:85-87 gate / up, :110-119 q / k / v).
 * B4 / sB / B8 / sB8 hold the `nseg` (1..3) weights concatenated along the output features: B4 [nseg * N_seg, K4/2], sB [G, nseg * N_seg]
 * flat, B8 [nseg * N_seg, 128], sB8 [nseg * N_seg].  Segment s gets its own output out_s [M, N_seg]: fp16, or the FP32 sums where bit s
 * of f32_mask is set (k / v ahead of atom_kv_quant_append_f32).  add0_f16 (optional, fp16 [M, N_seg]): added to segment 0's fp16
 * output as torch adds two half tensors -- half(float(half(c)) + float(add)) -- i.e. the decoder layer's residual add
 * (llama.py:268-275, :289-291) in the projection's own launch.  Per feature the arithmetic and the summation order are those of
 * atom_gemm_w4a4_f32 / of the decode-batch kernel behind atom_gemm_w4a4_f16: bit-identical to the separate launches (+ torch's add).
 * Shapes: atom_gemm_w4a4_multi_fits(M, N_seg, nseg, K_total) (decode batches; N_seg % 16 == 0); packed operands only.
 */
int atom_gemm_w4a4_multi_fits(int64_t M, int64_t N_seg, int nseg, int64_t K_total);
int atom_gemm_w4a4_multi(const void *A4, const void *B4, const void *sA, const void *sB, const void *A8, const void *B8,
                         const void *sA8, const void *sB8, void *out0, void *out1, void *out2, unsigned f32_mask,
                         const void *add0_f16, int64_t M, int64_t N_seg, int nseg, int64_t K_total, int group, int keeper,
                         int scale_layout, void *stream);

/*
 * atom_gemm_w4a4_multi with the quantiser that PRECEDES the GEMM inside the launch: one or two tokens of a decode step
 * (atom_gemm_w4a4_multi_q_fits).  The reference runs the two as separate ops -- punica/models/llama.py:259-263 input_layernorm
 * (rmsnorm_fp16_i4) -> :110-119 q / k / v; :176 reorder_fp16_i4 -> o_proj; :266-282 residual add + post_attention_layernorm -> :85
 * gate / up; :86 activate_fp16_i4 -> :87 down_proj -- and so does this library from three tokens on; at one or two tokens a
 * quantiser launch costs more than its arithmetic (a launch boundary, its own round trip through HBM, 4.4-4.7 us against the GEMM's 5-9), so
 * the GEMM launch quantises the token rows itself: once per CU, in front of the dot-product kernel's feature loop (round 6,
 * csrc/gemvq_w4a4.hip: one workgroup of 16 waves per CU; a Llama-7B decode layer at batch 1, cold, 60.8 -> 52 us with all four
 * quantisers inside).  (Rounds 3-5: in every 16-feature workgroup of the decode-batch kernel -- still the form for shapes the
 * dot-product form does not take.)
 *   q_op   ATOM_Q_REORDER      x [M, K_total] fp16, reorder_index (or NULL)           = atom_reorder_quant_f16
 *          ATOM_Q_RMSNORM      + x2 = the RMSNorm weight [K_total], eps               = atom_rmsnorm_reorder_quant_f16
 *          ATOM_Q_ADD_RMSNORM  + residual, residual_out [M, K_total] (x + residual)   = atom_add_rmsnorm_reorder_quant_f16
 *                              (NOT in place: every workgroup reads x and residual, workgroup 0 writes residual_out)
 *          ATOM_Q_SILU_MUL     x2 = the second factor [M, K_total]; no reorder index  = atom_silu_mul_quant_f16
 * in the kernel-flavoured arithmetic (quant_mode 0), clip as there.  Outputs, segments, f32_mask, add0_f16 as atom_gemm_w4a4_multi.
 * The quantised operand is bit-identical to the quantiser op's, and the sums are formed in the order atom_gemm_w4a4_multi uses for the
 * shape (atom_gemm_w4a4_packed_order: 64, the dot-product kernel's, for one token and for two with K_total > 4096 -- the quantiser then
 * sits in front of that kernel; 8, the decode-batch kernel's, for two tokens with K_total <= 4096): the outputs are bit-identical to the
 * quantiser op followed by atom_gemm_w4a4_multi (tests/test_gpu_e2e.py).  (Rounds 3-5 always summed in the decode-batch kernel's order
 * and were one fp16 ulp off where the separate call took the dot-product kernel.)
 */
#define ATOM_Q_REORDER 1
#define ATOM_Q_RMSNORM 2
#define ATOM_Q_ADD_RMSNORM 3
#define ATOM_Q_SILU_MUL 4
/* The same launch with the decode attention's KV-split merge in front of the reorder quantiser (round 6): `partials_f32` = the
 * workspace atom_batch_decode_append_i4 / atom_batch_decode_i4 filled when called with o == NULL -- float [M][heads][splits][130] =
 * 128 un-normalised values, the running maximum m (base 2) and the denominator d per (token, head, split), heads = K_total / 128 --
 * merged as the decode op's own merge launch does (out = sum_s o_s 2^(m_s - M) / sum_s d_s 2^(m_s - M), splits in order), rounded to
 * fp16, then reordered, quantised and multiplied as ATOM_Q_REORDER: bit-identical to batch_decode (merged) -> atom_gemm_w4a4_multi_q
 * (ATOM_Q_REORDER), two launch boundaries of a decode step fewer (the reference: punica/models/llama.py:168-196 batch_decode ->
 * reorder_fp16_i4 -> o_proj).  2 .. 16 splits, one or two tokens, M x K_total <= 8192: atom_gemm_w4a4_multi_merge_q_fits. */
int atom_gemm_w4a4_multi_merge_q_fits(int64_t M, int64_t N_seg, int nseg, int64_t K_total, int splits);
int atom_gemm_w4a4_multi_merge_q(const void *partials_f32, int splits, const int16_t *reorder_index, float clip, const void *B4, const void *sB,
                                 const void *B8, const void *sB8, void *out0, void *out1, void *out2, unsigned f32_mask,
                                 const void *add0_f16, int64_t M, int64_t N_seg, int nseg, int64_t K_total, int group, int keeper,
                                 void *stream);
/* 1 when atom_gemm_w4a4_multi_q takes (q_op, M, N_seg, nseg, K_total): the launcher's own predicate -- one or two tokens, K_total <=
 * 12,288 (three 4-channel quantiser tasks per thread of the 1024 and token row), for the three ops that stage fp16 rows and the norm
 * weight in LDS M x K_total <= 16,384, and a shape atom_gemm_w4a4_multi takes. */
int atom_gemm_w4a4_multi_q_fits(int q_op, int64_t M, int64_t N_seg, int nseg, int64_t K_total);
int atom_gemm_w4a4_multi_q(int q_op, const void *x, const void *x2, const void *residual, void *residual_out,
                           const int16_t *reorder_index, float eps, float clip, const void *B4, const void *sB, const void *B8,
                           const void *sB8, void *out0, void *out1, void *out2, unsigned f32_mask, const void *add0_f16, int64_t M,
                           int64_t N_seg, int nseg, int64_t K_total, int group, int keeper, void *stream);

/*
 * Same result contract, with an optional caller-owned scratch buffer for DECODE batches (the k/v projections of a
 * serving step; the shapes the decode-batch GEMM takes, M <= 256 at most).  The plain entry point runs the 256-row
 * tile kernel whatever M is (88 us at M = 16, N = K = 4096); with
 * a workspace of atom_gemm_w4a4_o4_workspace_bytes() bytes the weight-streaming decode kernel writes FP32 sums [M, N]
 * there and a second launch applies the u4 epilogue (same arithmetic; the FP32 summation order is the decode kernel's,
 * so a code can differ by one from the tile kernel's where a value sits on a rounding boundary).  0 bytes = the shape
 * does not use it; then, or with a NULL / too small workspace, this is atom_gemm_w4a4_o4.
 */
size_t atom_gemm_w4a4_o4_workspace_bytes(int64_t M, int64_t N, int64_t K_total);
int atom_gemm_w4a4_o4_ws(const void *A4, const void *B4, const void *sA, const void *sB,
                         const void *A8, const void *B8, const void *sA8, const void *sB8,
                         void *D_u4, void *D_scale_zero, int64_t M, int64_t N, int64_t K_total,
                         int group, int keeper, int scale_layout, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same sums WITHOUT the final rounding: D_f32 float [M, N] = the FP32 accumulators the u4 epilogue quantises.
 * Decode batches in the packed format only (the shapes the decode-batch GEMM takes; ATOM_ERR_SHAPE otherwise).  Feeds
 * atom_kv_quant_append_f32 below: k / v projection -> u4 codes -> paged cache in two launches per projection pair
 * instead of five.  No reference counterpart (its _o4 GEMM quantises in its epilogue, the append is a separate kernel).
 */
int atom_gemm_w4a4_f32(const void *A4, const void *B4, const void *sA, const void *sB,
                       const void *A8, const void *B8, const void *sA8, const void *sB8,
                       void *D_f32, int64_t M, int64_t N, int64_t K_total,
                       int group, int keeper, int scale_layout, void *stream);

/*
 * The three fused activation-quantisation ops.  Common outputs (row r, hidden = H, K4 = H-128):
 *   o_outliers     int8  [M, 128]        INT8 codes of the last 128 (reordered) channels
 *   o_norms        uint8 [M, K4/2]       packed INT4 codes of the first K4 channels
 *   outlier_scales fp16  atom_scale_size(M, layout) halves
 *   norm_scales    fp16  [K4/128, atom_scale_size(M, layout)]
 *   xq_f16         fp16  [M, H] or NULL  optional de-quantised tensor (codes*scale in half) == what the
 *                                         reference's quantize_activation_wrapper returns (sim mode)
 * Constraints: H % 128 == 0, 256 <= H <= 16384, reorder_index int16 [H] with values in [0,H); a NULL
 * reorder_index means the identity (input already in reordered channel order).
 */

/* y = index_select(x, -1, reorder_index); quantise.
 * Replaces: run_reorder_fp16_i4<128,4096> (kernels/include/Reorder/Reorder.cuh:205-228);
 * sim mode == index_select + quantize_activation_wrapper (model/qLlamaLayer.py:300-304). */
int atom_reorder_quant_f16(const void *x, const int16_t *reorder_index, int64_t M, int hidden,
                           int quant_mode, float clip, int scale_layout,
                           void *o_outliers, void *o_norms, void *outlier_scales, void *norm_scales,
                           void *xq_f16, void *stream);

/* y = RMSNorm(x)*w; index_select; quantise.
 * Replaces: run_rmsnorm_fp16_i4<128,4096> (kernels/include/RMSNorm/RMSNorm.cuh:255-285);
 * sim mode == QLlamaRMSNorm.forward (model/qLlamaLayer.py:141-151) with HF LlamaRMSNorm numerics. */
int atom_rmsnorm_reorder_quant_f16(const void *x, const void *weight, float eps,
                                   const int16_t *reorder_index, int64_t M, int hidden,
                                   int quant_mode, float clip, int scale_layout,
                                   void *o_outliers, void *o_norms, void *outlier_scales,
                                   void *norm_scales, void *xq_f16, void *stream);

/* NEW: residual_out[m,:] = x[m,:] + residual[m,:] (one fp16 add per element; residual_out may be
 * `residual` itself -- the residual stream of the decoder layer, llama.py:266-282), then exactly
 * atom_rmsnorm_reorder_quant_f16 of that sum.  Replaces the elementwise add kernel + the RMSNorm kernel's re-read of its
 * result (24 -> 16 KiB of HBM traffic per token at hidden 4096, one launch less). */
int atom_add_rmsnorm_reorder_quant_f16(const void *x, const void *residual, void *residual_out, const void *weight,
                                       float eps, const int16_t *reorder_index, int64_t M, int hidden,
                                       int quant_mode, float clip, int scale_layout,
                                       void *o_outliers, void *o_norms, void *outlier_scales,
                                       void *norm_scales, void *xq_f16, void *stream);

/* y = silu(a)*b; quantise (no reorder: the weights are pre-permuted, modelutils_llama.py:33-40).
 * Replaces: run_activate_fp16_i4<128,11008> (kernels/include/Activate/Activate.cuh:194-217);
 * sim mode == act_fn(gate)*up -> act_quant (model/qLlamaLayer.py:345-351). */
int atom_silu_mul_quant_f16(const void *a, const void *b, int64_t M, int hidden,
                            int quant_mode, float clip, int scale_layout,
                            void *o_outliers, void *o_norms, void *outlier_scales, void *norm_scales,
                            void *xq_f16, void *stream);

/*
 * NEW (the bridge the reference lacks): quantise + pack an FP16 weight [N,K] (columns
 * already reordered, keeper = last 128 columns) exactly as QLinearLayer.quant does
 * (model/qLinearLayer.py:42-78, model/quant.py:68-107): INT8 per output row for the keeper columns,
 * INT4 with `channel_group` (1 or 2) adjacent rows sharing a scale per 128-column slice, clip w_clip.
 * Outputs: B4 uint8 [N,K4/2], B8 int8 [N,128], sB fp16 [G,N], sB8 fp16 [N], Wq_f16 fp16 [N,K] or NULL
 * (the fake-quant weight the reference would hold).
 */
int atom_quant_weight_w4(const void *W_f16, int64_t N, int64_t K_total, float w_clip,
                         int channel_group, void *B4, void *B8, void *sB, void *sB8, void *Wq_f16,
                         void *stream);

/*
 * NEW (the bridge for GPTQ-written weights): pack a weight that is ALREADY fake-quantised -- every
 * value half(s*c) with c in [-8,7] sharing s per (`channel_group` rows x 128 columns), last 128 columns c in
 * [-128,127] with one s per row -- by recovering (c, s).  This is what GPTQ leaves in `layer.weight.data`
 * (model/gptq.py:38-39 quantises with an FP32 scale found on the error-compensated weight, :285-287, stores half(q),
 * :331, and discards the scale) and also what QLinearLayer.quant leaves (model/qLinearLayer.py:42-78; reproduced
 * exactly, the scale there is fp16).  For FP32-scale weights sB is the fp16 value that reproduces Wq best:
 * |c*sB - Wq| <= 2^-9 |Wq| + 2^-24 per element.  Outputs as atom_quant_weight_w4.  `bad_blocks` (device int32, may be
 * NULL) receives the number of blocks that are on no such grid; those are re-quantised round-to-nearest (the caller
 * decides whether that is an error -- the Python mirror raises).
 */
int atom_pack_weight_w4(const void *Wq_f16, int64_t N, int64_t K_total, int channel_group,
                        void *B4, void *B8, void *sB, void *sB8, int32_t *bad_blocks, void *stream);

/*
 * INT4 paged KV cache -- the two ops that follow the k/v projections (atom_gemm_w4a4_o4) in the
 * reference's decoder layer (e2e/punica-atom/punica/models/llama.py:196-211).  Layouts are the reference's
 * (punica/utils/kvcache.py:17-26, kernels/include/flashinfer/page.cuh:78-110):
 *   kv_data  uint8 [pages, num_layers, 2, num_heads, page_size, head_dim/2]  u4, element 2j in the low nibble
 *   kv_param fp16  [pages, num_layers, 2, num_heads, page_size, 2]           (scale, zero): value = u4*scale - zero
 *   kv_indptr int32 [batch+1], kv_indices int32 [kv_indptr[batch]], last_page_offset int32 [batch] (1..page_size);
 *   sequence b has (npages_b - 1)*page_size + last_page_offset[b] tokens.
 * head_dim must be 128 (as in the reference, punica_ops.cc:112), page_size a multiple of 16.
 */

/* Copy new tokens' quantised K/V (the d / d_scale outputs of atom_gemm_w4a4_o4, viewed [T, heads, 64] / [T, heads, 2])
 * into the pages.  append_indptr int32 [batch+1] (device): the tokens are the LAST append_indptr[b+1]-append_indptr[b]
 * positions of sequence b (pages already allocated, lengths already updated), total_tokens = append_indptr[batch];
 * append_indptr == NULL: one token per sequence (total_tokens == batch).
 * Replaces: FlashInferInitKvKernel_i4 / FlashInferAppendKvKernel_i4 (punica/ops/csrc/flashinfer_adapter/
 * flashinfer_impl.cuh:48-96; page.cuh:119-227) = punica_ops.cc:122-209 init_kv_i4 / append_kv_i4. */
int atom_kv_append_i4(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                      const int32_t *last_page_offset, const void *k, const void *v, const void *k_param,
                      const void *v_param, const int32_t *append_indptr, int64_t total_tokens, int batch,
                      int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, void *stream);

/* Decode step, fused: quantise the FP32 sums of the k / v projections (atom_gemm_w4a4_f32: float [batch, heads*128] each)
 * per head with the arithmetic of the _o4 epilogue (DenseLayerGEMM_i4_o4.cu:704-788) and write codes + (scale, zero)
 * into the LAST token's slot of each sequence (the one-token-per-sequence form of FlashInferAppendKvKernel_i4,
 * flashinfer_impl.cuh:72-96).  Bit-identical cache contents to atom_gemm_w4a4_o4_ws + atom_kv_append_i4. */
int atom_kv_quant_append_f32(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                             const int32_t *last_page_offset, const void *k_f32, const void *v_f32, int batch,
                             int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, void *stream);

/* o[b,h,:] (fp16) = softmax_j( <RoPE(q[b,h], len_b-1), RoPE(dequant K[b,h,j], j)> / sqrt(128) ) . dequant V[b,h,j].
 * Replaces: FlashInferBatchDecodeKernel_i4 (flashinfer_impl.cuh:9-46; decode.cuh:480-676) = punica_ops.cc:82-120
 * batch_decode_i4 (rope_theta 1e4, rope_scale 1 there).  max_pages_per_seq (host-side upper bound of npages_b, 0 =
 * unknown) lets long sequences at small batch split their KV range over several waves: FP32 partial states go to
 * `workspace` (atom_batch_decode_i4_workspace_bytes; NULL / too small = no split) and a second launch merges them.  Where
 * batch x num_heads >= 256 and the split count divides 12 (round 6) the splits are waves of one workgroup instead and merge in LDS:
 * one launch, the workspace is not touched, the same bits. */
size_t atom_batch_decode_i4_workspace_bytes(int batch, int num_heads, int page_size, int max_pages_per_seq);
/* ... how many PARTIAL STATES per (sequence, head) the call produces for these arguments (1 = none: no workspace use).  At small batches
 * the waves that share a pair's KV range come in workgroups of four that leave one partial state each (round 6), so this is the
 * number of such workgroups, not of waves.  With o == NULL and a
 * split count >= 2 the two decode entry points leave the partial states in the workspace UN-merged, as float [batch][heads][splits][130]
 * (128 un-normalised values, running maximum, denominator), for a consumer that merges them itself: atom_gemm_w4a4_multi_merge_q. */
int atom_batch_decode_i4_splits(int batch, int num_heads, int page_size, int max_pages_per_seq);
int atom_batch_decode_i4(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                         const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers,
                         int layer_idx, int num_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                         int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream);
/* atom_kv_quant_append_f32 + atom_batch_decode_i4 of a pure decode step in ONE launch (round 6): k_f32 / v_f32 (float [batch, heads*128])
 * are this step's k / v projections; for every (sequence, head) the wave that attends to the last token quantises them (the same _o4
 * arithmetic), writes codes + (scale, zero) into the last token's cache slot and attends to the values it has just written -- the
 * reference's call order punica/models/llama.py:168-196 (append_kv, then batch_decode) with bit-identical cache contents and output,
 * without the launch boundary between the two. */
int atom_batch_decode_append_i4(void *o, const void *q, const void *k_f32, const void *v_f32, void *kv_data, void *kv_param,
                                const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset, int batch,
                                int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, float rope_theta,
                                float rope_scale, int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream);

/* Prefill / chunked-prefill attention over the same cache: causal multi-query attention, RoPE fused.  Sequence b's queries are rows
 * qo_indptr[b] .. qo_indptr[b+1] of q (fp16 [total_q, heads, 128], not yet rotated; qo_indptr int32 [batch+1] on the device) and
 * sit at the LAST q_b positions of its len_b cached tokens (the tokens atom_kv_append_i4 has just written there): query i at
 * p = len_b - q_b + i, attending to keys 0 .. p.
 *   o[row,h,:] (fp16) = softmax_{j <= p}( <RoPE(q[row,h], p), RoPE(dequant K[b,h,j], j)> / sqrt(128) ) . dequant V[b,h,j]
 * With one query per sequence this is atom_batch_decode_i4.  q, the rotated keys, the softmax weights and the de-quantised values
 * are rounded to fp16 as matrix-core operands (FP32 accumulation, FP32 softmax): the only departure from the FP32 arithmetic of
 * the decode op.  Cache slots past a sequence's end are never read.
 * max_q_len: host-side bound of every q_b (it sizes the grid; a sequence with more queries is an error the op cannot see);
 * max_pages_per_seq (0 = unknown) lets few query blocks on long prefixes split their KV range: FP32 partial states go to
 * `workspace` (atom_batch_prefill_i4_workspace_bytes; NULL / too small = no split) and a second launch merges them.
 * Errors: ATOM_ERR_INVALID_ARG for a null pointer (o, q, qo_indptr or a cache table), rope_theta <= 0 or rope_scale <= 0;
 * ATOM_ERR_SHAPE for head_dim != 128, page_size not a multiple of 16, a layer out of range, batch / num_heads < 1, total_q < 1
 * or max_q_len < 1; ATOM_ERR_ALIGN for q / o / kv_data not 16-byte aligned or kv_param / qo_indptr not 4-byte aligned. */
size_t atom_batch_prefill_i4_workspace_bytes(int64_t total_q, int batch, int num_heads, int page_size, int max_q_len,
                                             int max_pages_per_seq);
int atom_batch_prefill_i4(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                          const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                          int batch, int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, float rope_theta,
                          float rope_scale, int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream);

/* Grouped-query attention (GQA) over the same cache: the cache holds num_kv_heads heads, q / o are fp16 [rows, num_qo_heads, 128],
 * and query head h reads K/V head h / G, G = num_qo_heads / num_kv_heads (HF's repeat_kv).  Decode and prefill compute what the two
 * entry points above compute on the cache with every K/V head repeated G times, without that copy: a workgroup serves a (sequence,
 * K/V head) pair -- or a query block of it -- for all G query heads of the group, so each K/V tile is read from memory and
 * de-quantised once per group (csrc/prefill_i4.hip, batch_prefill_kernel<true>).
 * Numerics of BOTH entry points are the prefill op's: q, the rotated keys, the softmax weights and the de-quantised values are rounded
 * to fp16 as matrix-core operands, FP32 accumulation and softmax (the GQA decode op is the prefill kernel with one query per sequence).
 * num_qo_heads == num_kv_heads: the calls forward to atom_batch_decode_i4 / atom_batch_prefill_i4 (their bits, workspace sizes and
 * split counts).  The decode op's partial states (o == NULL, splits >= 2) keep the layout float [batch][num_qo_heads][splits][130], for
 * atom_gemm_w4a4_multi_merge_q; its split count is sized by batch x num_kv_heads.
 * Errors: those of the MHA entry points, and ATOM_ERR_SHAPE for num_kv_heads < 1, num_qo_heads < 1 or num_qo_heads % num_kv_heads != 0
 * (checked before any pointer; the size queries return 0 there).  The cache's K/V are appended by atom_kv_append_i4 /
 * atom_kv_quant_append_f32 with num_heads = num_kv_heads. */
size_t atom_batch_decode_gqa_i4_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq);
int atom_batch_decode_gqa_i4_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq);
int atom_batch_decode_gqa_i4(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                             const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                             int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                             int max_pages_per_seq, void *workspace, size_t workspace_bytes, void *stream);
size_t atom_batch_prefill_gqa_i4_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                 int max_q_len, int max_pages_per_seq);
int atom_batch_prefill_gqa_i4(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                              const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                              int batch, int num_layers, int layer_idx, int num_qo_heads, int num_kv_heads, int page_size, int head_dim,
                              float rope_theta, float rope_scale, int max_pages_per_seq, void *workspace, size_t workspace_bytes,
                              void *stream);

/* RoPE scaling (Llama 3.1 / 3.2 "llama3", YaRN): the three entry points above with a per-pair FREQUENCY TABLE and an ATTENTION SCALE,
 * inserted behind rope_scale; every other argument, the plan queries (*_workspace_bytes, *_splits) and the partial states (o == NULL)
 * are the parent's.
 *   rope_table  device float[64], 4-byte aligned: the frequency of RoPE pair i (dims i, i + 64) in REVOLUTIONS per position, i.e.
 *               inv_freq_i / (2 pi).  The kernels use it as loaded -- nothing multiplies it -- so the angle of position p is
 *               2 pi * p * rope_table[i] with the fp32 table value taken exactly: the table is its own definition.  With a table
 *               rope_theta and rope_scale are checked as before and otherwise ignored.  The launch reads exactly 64 floats; bad values
 *               (NaN, Inf, negative) give a wrong answer, never a fault.  The product p * rope_table[i] is formed exactly (p as a float:
 *               exact below 2^24) before its fractional part is taken -- in the prefill / grouped-query kernel for the query always
 *               and for keys from position 8192 on (below it the rounded product is off by < 1e-4 revolution) --, so positions of
 *               131,072 cost no accuracy.
 *   attn_scale  multiplies the logits (folded into the softmax scale on the host); YaRN passes attention_factor^2.
 * Contract: rope_table == NULL and attn_scale == 1.0f give the parent entry point's bits (the same kernels, launch for launch) and
 * the parent's error codes.  A call whose only faults are in the parent's arguments returns the parent's code, in the parent's order;
 * the new faults are reported behind ALL of those: attn_scale not greater than 0 (or NaN) ATOM_ERR_INVALID_ARG, then a table that
 * is not 4-byte aligned ATOM_ERR_ALIGN.  num_qo_heads == num_kv_heads: the grouped-query entries run the MHA kernels, as their parents. */
int atom_batch_decode_gqa_i4_rope(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                  const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                  int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                  size_t workspace_bytes, void *stream);
int atom_batch_prefill_gqa_i4_rope(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                   const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                   const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                   int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                   const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                   size_t workspace_bytes, void *stream);
int atom_batch_decode_append_i4_rope(void *o, const void *q, const void *k_f32, const void *v_f32, void *kv_data, void *kv_param,
                                     const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset, int batch,
                                     int num_layers, int layer_idx, int num_heads, int page_size, int head_dim, float rope_theta,
                                     float rope_scale, const float *rope_table, float attn_scale, int max_pages_per_seq, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* Sliding-window attention (Mistral-7B-v0.1, "sliding_attention" layers): the grouped-query _rope entry points with `window` inserted
 * behind attn_scale, and their plan queries with `window` as the last argument.
 *   - window = W >= 1: the query at position p sees the keys j with p - W < j <= p -- W keys including its own (HF's
 *     kv_idx > q_idx - sliding_window).
 *   - The bound is per query row, from that row's own position: not from its chunk's first row, not from the sequence's end.
 *   - A sequence no longer than W gets plain causal attention.
 *   - RoPE (rope_theta / rope_scale / rope_table), attn_scale, the head mapping h -> h / G and the paging are the _rope entries'.
 *   - Pages behind the window stay allocated and are not read: the call frees nothing.
 * Both entries run the matrix-core kernel (csrc/prefill_i4.hip, the kWindow instantiations) at EVERY head ratio, num_qo_heads ==
 * num_kv_heads included -- nothing forwards to the FP32 decode op -- so their numerics are the grouped-query ops' and their plan is
 * the grouped-query plan: the split policies see the most 64-key tiles a query block can touch under the window (never more than the
 * cache holds: a window that covers max_pages_per_seq * page_size keys plans as the un-windowed grouped-query op).  Query blocks split
 * the tiles from their first row's lowest key on; a split that gets no tile writes the empty state (m = -inf, l = 0).
 * o == NULL (decode entry, splits >= 2) leaves the partial states float [batch][num_qo_heads][splits][130] un-merged, for
 * atom_gemm_w4a4_multi_merge_q; splits is atom_batch_decode_gqa_i4_win_splits with the same arguments.
 * Errors: every fault of the _rope entries, in their order; behind ALL of them window < 1 is ATOM_ERR_INVALID_ARG.  The queries
 * return 0 for window < 1 and for the inputs their parents reject. */
size_t atom_batch_decode_gqa_i4_win_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq,
                                                    int window);
int atom_batch_decode_gqa_i4_win_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq, int window);
size_t atom_batch_prefill_gqa_i4_win_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                     int max_q_len, int max_pages_per_seq, int window);
int atom_batch_decode_gqa_i4_win(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                 const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                 int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                 const float *rope_table, float attn_scale, int window, int max_pages_per_seq, void *workspace,
                                 size_t workspace_bytes, void *stream);
int atom_batch_prefill_gqa_i4_win(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                  const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                  const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                  int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int window, int max_pages_per_seq, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* Sliding-window attention over a ROLLING cache: the _win entry points with `kv_start` inserted behind window.
 *   kv_start int32 [batch] on the device: the position of the first token of sequence b's page list -- what atom_kv_step_ring_i4
 *   writes.  The pages behind the window have been released; the list holds the live ones in logical order.
 *   - start = kv_start[b] is a multiple of page_size, not necessarily of 64.
 *   - The sequence's length is start + (pages - 1) * page_size + last_page_offset.
 *   - Everything else stays in ABSOLUTE positions: the positions of the queries (the LAST q_b of that length), the causal and the
 *     window bound, the 64-key tile grid, the KV splits and the RoPE angle of key j.  Given equal contents and an equal split count the
 *     call performs the operations of the _win call on a cache that released nothing, in the same order: the results are bit-identical.
 *   - Key j is read from page (j - start) / page_size of the list.  Keys with j < start or j >= length are not loaded; they are
 *     staged as zeros.
 *   - The caller guarantees start <= p - window + 1 for every query position p (atom_kv_step_ring_i4 does), so the window bound
 *     already masks every key below start.  A caller that breaks the guarantee gets an unspecified finite result; no value of
 *     kv_start makes the kernel read outside the listed pages.
 * Plan: max_pages_per_seq is the ring's size R, and a list of R * page_size tokens that starts off a 64-key boundary touches up to
 * (R * page_size + 62) / 64 + 1 tiles, one more than the _win plan assumes for that many pages -- so these entries have plan queries of
 * their own, with the _win queries' arguments.  For a ring of at least ceil((window - 1 + q_b) / page_size) + 1 pages the window
 * bound governs and the plan is the _win call's at a large max_pages_per_seq.  The partial-state layout is unchanged (o == NULL on the
 * decode entry feeds atom_gemm_w4a4_multi_merge_q).
 * Errors: every fault of the _win entries, in their order; behind ALL of them a null kv_start is ATOM_ERR_INVALID_ARG, one that is not
 * 4-byte aligned ATOM_ERR_ALIGN. */
size_t atom_batch_decode_gqa_i4_ring_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq,
                                                     int window);
int atom_batch_decode_gqa_i4_ring_splits(int batch, int num_qo_heads, int num_kv_heads, int page_size, int max_pages_per_seq, int window);
size_t atom_batch_prefill_gqa_i4_ring_workspace_bytes(int64_t total_q, int batch, int num_qo_heads, int num_kv_heads, int page_size,
                                                      int max_q_len, int max_pages_per_seq, int window);
int atom_batch_decode_gqa_i4_ring(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                                  const int32_t *kv_indices, const int32_t *last_page_offset, int batch, int num_layers, int layer_idx,
                                  int num_qo_heads, int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                  const float *rope_table, float attn_scale, int window, const int32_t *kv_start, int max_pages_per_seq,
                                  void *workspace, size_t workspace_bytes, void *stream);
int atom_batch_prefill_gqa_i4_ring(void *o, const void *q, const int32_t *qo_indptr, int64_t total_q, int max_q_len, const void *kv_data,
                                   const void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                   const int32_t *last_page_offset, int batch, int num_layers, int layer_idx, int num_qo_heads,
                                   int num_kv_heads, int page_size, int head_dim, float rope_theta, float rope_scale,
                                   const float *rope_table, float attn_scale, int window, const int32_t *kv_start, int max_pages_per_seq,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* Page tables stepped on the device (csrc/kv_step.hip): rebuilds kv_indptr / kv_indices / last_page_offset -- the layout above, what
 * every attention and append entry point reads -- in ONE launch from buffers at fixed addresses, so that a captured decode step can
 * be replayed for the next token with no host work in between.
 *   page_table int32 [batch, cap]  the pages reserved for each sequence, in order (read only)
 *   row_pages  int32 [batch]       how many entries of each row are reserved pages (read only; clamped into 0 .. cap); the entries
 *                                  behind them are never copied
 *   lens       int32 [2, batch]    the lengths, double-buffered: row (state[1] & 1) is current; the launch writes the other row and
 *                                  flips state[1] (every workgroup reads all current lengths, so they cannot be updated in place)
 *   state      int32 [4]           [0] status bits, only ever SET by the launch (the caller reads and clears them);
 *                                  [1] parity of `lens`; [2] the launch's arrival counter, 0 between launches; [3] unused.  Zero it once.
 *   kv_indptr int32 [batch+1], kv_indices int32 [batch * cap] (the first kv_indptr[batch] are meaningful), last_page_offset int32 [batch]
 * Sequence b's new length is len_b + add (add = 1: a decode step; add = 0: rebuild the tables of the current lengths) unless that
 * needs more than row_pages[b] pages: then it keeps its length and ATOM_KV_STEP_OVERFLOW is set.  A stored length outside
 * 0 .. row_pages[b] * page_size is clamped into that range and ATOM_KV_STEP_BAD_LENGTH is set.  So no page count above a sequence's
 * reserve (hence none above `cap`) and no index from outside its row ever reaches the tables: capacity is an error the caller reads later, never a fault.  An empty sequence has no page and
 * last_page_offset 0.  Launches that share buffers must be ordered on the device (one stream, or a captured chain).
 * Errors: ATOM_ERR_INVALID_ARG for a null pointer or add < 0; ATOM_ERR_SHAPE for batch < 1, cap < 1, page_size not a multiple of 16,
 * cap * page_size or batch * cap beyond int32; ATOM_ERR_ALIGN for a pointer that is not 4-byte aligned. */
#define ATOM_KV_STEP_OVERFLOW 1
#define ATOM_KV_STEP_BAD_LENGTH 2
int atom_kv_step_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                    int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, int add, void *stream);

/* The same step with a count per sequence and a look-ahead (speculative decoding; the same kernel body):
 *   adds int32 [batch] on the device: sequence b gains adds[b] tokens; lookahead >= 0.
 * The COMMITTED length len_b + adds[b] is what `lens` receives; kv_indptr / kv_indices / last_page_offset are built for the committed
 * length + lookahead.  The `lookahead` slots behind the committed length are tentative: a verify step writes its K + 1 tokens there, the
 * next launch commits the accepted ones through adds, and the others are overwritten.  Nothing is ever rolled back.
 * adds[b] < 0 counts as 0 and sets ATOM_KV_STEP_BAD_LENGTH.  If len_b + adds[b] + lookahead exceeds the sequence's reserve, the whole
 * request is refused as above: the sequence keeps len_b, its tables are those of len_b, and ATOM_KV_STEP_OVERFLOW is set.  With
 * lookahead 0 and every adds[b] = add the result is atom_kv_step_i4's.  Both entries flip the parity once per launch and may be mixed.
 * Errors: as atom_kv_step_i4, with ATOM_ERR_INVALID_ARG for a null adds or lookahead < 0 and ATOM_ERR_ALIGN for adds off 4 bytes. */
int atom_kv_step_rows_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                         int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, const int32_t *adds, int lookahead,
                         void *stream);

/* The step over a RING of pages (rolling cache of a sliding-window model; the same kernel body): the arguments of
 * atom_kv_step_i4 plus `window` = W >= 1 and an output kv_start int32 [batch].
 *   - page_table[b][0 .. R), R = min(row_pages[b], cap), is a ring: logical page g of sequence b (tokens g * page_size ..
 *     g * page_size + page_size - 1) lives in slot g % R.  `lens` stays the ABSOLUTE length, double-buffered as above; `state` as above.
 * For the new length n = len_b + add:
 *   - first live logical page f = max(0, n - max(add, 1) - W + 1) / page_size: the lowest key that the oldest of the step's new rows
 *     still sees, floored to a page;
 *   - last live logical page l = (n + page_size - 1) / page_size - 1; the page count is cnt = l - f + 1, 0 for an empty sequence;
 *   - cnt > R: the sequence is NOT advanced, its tables are those of its old length (the pages f .. l of n = len_b, add = 0) and
 *     ATOM_KV_STEP_OVERFLOW is set -- a status bit, never a fault;
 *   - a stored length below 0 or above 0x7fffffff - add is clamped into that range and ATOM_KV_STEP_BAD_LENGTH is set; a stored
 *     length whose own pages exceed R is flagged too and listed by its last R pages (none for R = 0: the sequence is then empty).  No
 *     page count above R and no index from outside a row ever reaches kv_indices.
 * Outputs: kv_indptr, the exclusive prefix sum of cnt; kv_indices in LOGICAL order, entry j of sequence b = page_table[b][(f + j) % R];
 * last_page_offset = (n - 1) % page_size + 1 (0 when empty); kv_start[b] = f * page_size (what the _ring attention entries take).
 * Why a slot may be reused: the page that receives token n - 1 sits in slot l % R; that slot's previous tenant was logical page
 * l - R < f, which is no longer listed.  The bytes of the slot beyond n are stale and are never read: the attention kernels stop at
 * the length.  There is no ring form of atom_kv_step_rows_i4.
 * Errors: as atom_kv_step_i4, with ATOM_ERR_INVALID_ARG for window < 1 or a null kv_start and ATOM_ERR_ALIGN for a kv_start off 4 bytes. */
int atom_kv_step_ring_i4(const int32_t *page_table, const int32_t *row_pages, int32_t *lens, int32_t *kv_indptr, int32_t *kv_indices,
                         int32_t *last_page_offset, int32_t *state, int batch, int cap, int page_size, int add, int window,
                         int32_t *kv_start, void *stream);

/*
 * KV-cache fake quantisation of the simulated path: every 128-d head vector of x is quantised
 * asymmetrically to n_bits in FP16 opmath -- scale = ((max - min) * clip).clamp(1e-5) / (2^n - 1), base =
 * round(-min / scale).clamp(0, 2^n - 1), y = (clamp(round(x / scale) + base, 0, 2^n - 1) - base) * scale -- and written
 * back as fp16.  Replaces: quantize_attn_k_wrapper / quantize_attn_v_wrapper (model/quant.py:233-257 ->
 * quantize_tensor(sym=False), :143-145,173-181).  x is a [batch, num_heads, seq_len, 128] view with the given ELEMENT
 * strides (last dim contiguous; the reference feeds the transposed projection output), y is contiguous; y == x is
 * allowed when x is contiguous.
 */
int atom_kv_fake_quant_f16(const void *x, void *y, int64_t batch, int num_heads, int64_t seq_len, int64_t stride_b,
                           int64_t stride_h, int64_t stride_s, int n_bits, float clip, void *stream);

/* Rows per group of an F6 operand buffer: `rows` rounded up to 256 (buffer bytes = G * atom_f6_rows(rows) * 104). */
size_t atom_f6_rows(int64_t rows);

/* Packed INT4 weights B4 [N, K4/2] -> the F6 format (see ATOM_AB_F6): B_f6 uint8 [G][atom_f6_rows(N)][104], pad rows and
 * bytes 96..103 zeroed.  Offline, once per weight. */
int atom_repack_weight_f6(const void *B4, int64_t N, int64_t K_total, void *B_f6, void *stream);

/* Packed INT4 activations A4 [M, K4/2] + their scales sA (per `scale_layout`) -> the F6 activation operand [G][atom_f6_rows(M)][104]
 * with the token scales in the rows (what ATOM_QUANT_F6_CODES makes the quantisers emit directly; this is for callers that hold the
 * reference's packed format, e.g. ahead of atom_gemm_w4a4_silu_mul_quant_f6).  One bandwidth-bound launch. */
int atom_repack_act_f6(const void *A4, const void *sA, int64_t M, int64_t K_total, int scale_layout, void *A_f6, void *stream);

/* The same + the fp16 weight scales sB [G, N] appended as float32 [G][atom_f6_rows(N)] (ATOM_B_F6S): B_f6s holds
 * atom_f6_weight_bytes(N, K_total) = G * atom_f6_rows(N) * (104 + 4) bytes. */
size_t atom_f6_weight_bytes(int64_t N, int64_t K_total);
int atom_repack_weight_f6s(const void *B4, const void *sB, int64_t N, int64_t K_total, void *B_f6s, void *stream);

/*
 * gate_proj + up_proj + act_fn(gate) * up + the per-token group quantiser in ONE launch: what the reference runs as
 * two dense_layer_gemm_i4_fp16 calls and activate_fp16_i4 (punica/models/llama.py:85-87; model/qLlamaLayer.py:345-351).  A_f6 is the
 * F6 activation operand [G][atom_f6_rows(M)][104]; Bgu_f6s is the F6 weight buffer WITH appended fp32 scales
 * (atom_repack_weight_f6s) of the 2 * N_inter fused rows: per block j of 128 features and quarter w = 0..3, gate rows
 * 128 j + 32 w .. + 31 followed by the same 32 up rows; Bgu8 int8 [2 N_inter, 128] and sBgu8 fp16 [2 N_inter] in the same row
 * order.  Outputs = atom_silu_mul_quant_f16's with ATOM_QUANT_F6_CODES, for hidden N_inter: o_outliers int8 [M, 128], o_norms_f6
 * uint8 [N_inter / 128 - 1][atom_f6_rows(M)][104] (the F6 activation operand of down_proj), outlier_scales / norm_scales per
 * `scale_layout`, optional xq fp16 [M, N_inter] (NULL: not written).  quant_mode ATOM_QUANT_SIM / ATOM_QUANT_KERNEL, clip as there.
 * The K steps are summed in order (fp16 GEMM outputs are formed in registers and go through the same arithmetic): bit-identical to
 * the three launches it replaces wherever atom_gemm_w4a4_f6_order(M, N_inter, K_total) == 1 (every shape that fills the chip); for
 * few-tile shapes, where the stand-alone GEMMs add two / four ordered K ranges, same tolerance instead (the module wrappers fuse only
 * in the first case).  Saves writing and re-reading 2 * M * N_inter fp16.  Always the 256x256 geometry: meant for prefill batches (M >= 512).
 * N_inter % 128 == 0, N_inter >= 256; K_total as atom_gemm_w4a4_f16.
 */
int atom_gemm_w4a4_silu_mul_quant_f6(const void *A_f6, const void *Bgu_f6s, const void *A8, const void *Bgu8, const void *sA8,
                                     const void *sBgu8, int64_t M, int64_t N_inter, int64_t K_total, int group, int keeper,
                                     int quant_mode, float clip, int scale_layout, void *o_outliers, void *o_norms_f6,
                                     void *outlier_scales, void *norm_scales, void *xq, void *stream);

/*
 * Sparse mixture of experts (Mixtral) on the W4A4 path -- csrc/moe_w4a4.hip; no reference kernels: the reference runs the block as a
 * Python loop over the experts with a host read per expert (model/qMixtralLayer.py:302-350).  Three launches with no host work between
 * them.  T tokens, E experts, R = T * top_k routed rows.
 *
 * atom_moe_route_topk: the routing tables of logits fp16 [T, E] in ONE launch (one workgroup), all outputs on the device:
 *   topk_ids      int32 [T, top_k]  the experts with the top_k largest logits, largest first; of equal logits the LOWER expert index wins
 *   topk_w        fp16  [T, top_k]  w_k = exp(l_k - l_max) / sum_{j selected} exp(l_j - l_max) in FP32, rounded to fp16 (= softmax, topk,
 *                                   renormalise, .to(half) of qMixtralLayer.py:313-317: the full softmax's denominator cancels)
 *   expert_indptr int32 [E + 1]     rows per expert, prefix-summed
 *   row_token     int32 [R]         the token of each routed row: rows grouped by expert, ascending token order within an expert --
 *                                   by construction (ballot ranks and prefix sums), never by the order of atomics
 *   slot_row      int32 [T, top_k]  the row that holds slot (t, k)
 *   tile_expert, tile_row0 int32 [atom_moe_max_tiles(R, E)]  the tile table: for each expert in order, one tile per started 64 rows
 *                                   (entries from n_tiles on are not written)
 *   n_tiles       int32 [1]
 * atom_moe_max_tiles(R, E) = R / 64 + min(E, R) bounds n_tiles for any routing (host function).
 * Errors: ATOM_ERR_INVALID_ARG for a null pointer; ATOM_ERR_SHAPE unless 2 <= E <= 64, 1 <= top_k <= min(8, E), T >= 1, R < 2^31;
 * ATOM_ERR_ALIGN for a table that is not 4-byte aligned.
 *
 * atom_moe_gemm_w4a4_f16: the routed ("grouped") GEMM.  For every routed row r of expert e (expert_indptr[e] <= r < expert_indptr[e+1])
 * and feature n:  D[r, n] = contract(A[row_index ? row_index[r] : r], B_e[n])  with exactly the arithmetic of atom_gemm_w4a4_f16 in
 * tile-kernel order (atom_gemm_w4a4_packed_order == 1): bit-identical to that entry point on the expert's gathered rows, whatever tile
 * a row lands in.  Packed reference format only: A4 uint8 [A_rows, K4/2], A8 int8 [A_rows, 128], sA / sA8 per `scale_layout` (REF or
 * PLAIN) over A_rows rows and indexed by the SOURCE row (the gather applies to the scales too); stacked weights B4 uint8 [E, N, K4/2],
 * B8 int8 [E, N, 128], sB fp16 [E, G, N], sB8 fp16 [E, N]; row_index int32 [R] (values in 0 .. A_rows - 1) or NULL = the identity; the
 * tables of atom_moe_route_topk (or any tables of that form).  N = nseg * N_seg features (nseg 1 or 2): segment s goes to its own
 * contiguous out_s fp16 [R, N_seg] (gate and up of one launch, ready for atom_silu_mul_quant_f16).  Rows >= R of the outputs are never
 * written.  Grid: atom_moe_max_tiles(R, E) * (N / 64) workgroups, sized on the host from R alone; workgroups beyond *n_tiles leave
 * before touching memory.  64 x 64 tiles over the whole K range (the kernel of gemm_w4a4_mid.hip with the tile looked up).
 * Constraints: N_seg % 64 == 0, K_total as atom_gemm_w4a4_f16, 1 <= E <= 64, 1 <= R < 2^31, A_rows * K4/2 < 2^32 and N * K4/2 < 2^32
 * (32-bit lane offsets); ATOM_ERR_SHAPE otherwise; null pointers / a bad layout ATOM_ERR_INVALID_ARG; ATOM_ERR_ALIGN as there.
 *
 * atom_moe_combine_f16: out[t, :] = residual[t, :] + sum_k half(y[slot_row[t, k], :] * topk_w[t, k]), y fp16 [R, H]: the slots of a
 * token are added in ASCENDING EXPERT ID into an fp16 accumulator that starts at zero, every add as torch adds two half tensors --
 * half(float(a) + float(b)) --, the residual last (NULL: none): expert(x) * routing_weight, index_add_ into zeros in expert order,
 * residual + hidden of qMixtralLayer.py:344-348, :434.  H % 8 == 0 (16-byte loads and stores), top_k <= 8.
 */
int64_t atom_moe_max_tiles(int64_t R, int E);
int atom_moe_route_topk(const void *logits, int64_t T, int E, int top_k, int32_t *topk_ids, void *topk_w, int32_t *expert_indptr,
                        int32_t *row_token, int32_t *slot_row, int32_t *tile_expert, int32_t *tile_row0, int32_t *n_tiles, void *stream);
int atom_moe_gemm_w4a4_f16(const void *A4, const void *B4, const void *sA, const void *sB, const void *A8, const void *B8,
                           const void *sA8, const void *sB8, const int32_t *row_index, const int32_t *expert_indptr,
                           const int32_t *tile_expert, const int32_t *tile_row0, const int32_t *n_tiles, void *out0, void *out1,
                           int64_t A_rows, int64_t R, int E, int64_t N_seg, int nseg, int64_t K_total, int group, int keeper,
                           int scale_layout, void *stream);
int atom_moe_combine_f16(const void *y, const int32_t *slot_row, const int32_t *topk_ids, const void *topk_w, const void *residual,
                         void *out, int64_t T, int top_k, int64_t H, void *stream);

/*
 * Multi-adapter LoRA on fp16 activations beside the 4-bit base -- csrc/lora_f16.hip (the reference's punica.ops bgmv / add_lora,
 * e2e/punica-atom/punica/ops/__init__.py:62-124, whose kernels it no longer compiles), generalised from rows to row SEGMENTS.
 *
 * atom_bgmv_f16: for every segment s -- rows seg_indptr[s] .. seg_indptr[s+1]-1, or row s when seg_indptr is NULL -- with adapter
 * a = seg_adapter[s]:
 *     a < 0 or a >= capacity:  the segment's rows of y are not touched (an id is never turned into an address unless 0 <= a < capacity)
 *     else:  y[i, n] = half( float(y[i, n]) + scale * SUM_h float(x[i, h]) * float(W[a, layer_idx, n, h]) )
 *   x fp16 [rows, H1]; y fp16 [rows, H2], updated in place; W fp16 [capacity, L, H2, H1]; seg_adapter int32 [S] and seg_indptr int32
 *   [S + 1] (or NULL) on the device.  FP32 accumulation in the kernel's own (fixed) order, ONE rounding to fp16, at the store.  Rows at
 *   or beyond seg_indptr[S] (and beyond `rows`) are never written; an empty segment costs nothing.  One of H1, H2 is the adapter rank --
 *   a multiple of 8 in 8 .. 64 --, the other a multiple of 64 (or a rank too).  Two regimes: with a segment table, 16-row tiles of one
 *   segment on v_mfma_f32_16x16x32_f16 (a tile across a segment's end masks its rows), a grid of rows / 16 + S row tiles sized on the
 *   host, every workgroup finding its segment in the device table and leaving before it touches memory when it has none; without
 *   one (decode: a row per segment) dot-product kernels.  One thread writes an output element, no atomics, no split of the h sum
 *   across workgroups: a row's result depends on nothing but that row, its adapter and the shapes.  No host read, no
 *   synchronisation: capturable.
 * atom_add_lora_f16: y += scale * half(x A_a^T) B_a^T as two such passes: t[i, :] = half(SUM_h x[i, h] A[a, layer_idx, :, h]) into the
 *   caller's fp16 workspace t [rows, rank] (written, not added to: the "zeroed t, scale 1" of the reference; rows of segments without
 *   an adapter keep what t held and are not read), then y[i, n] = half(float(y[i, n]) + scale * SUM_j float(t[i, j]) B[a, layer_idx, n, j]).
 *   Without a segment table (one-row segments) both passes run in ONE launch, t rounded to fp16 in LDS and the caller's t untouched:
 *   the same operations in the same order, so the same bits as two atom_bgmv_f16 calls (the first into a zeroed t with scale 1).
 *   A = wa fp16 [capacity, L, rank, H1], B = wb fp16 [capacity, L, H2, rank]; H1 % 64 == 0, H2 % 64 == 0, rank % 8 == 0 in 8 .. 64.
 * Errors of both (all checked before any launch): ATOM_ERR_INVALID_ARG for a null y, x, weight, seg_adapter or t; ATOM_ERR_SHAPE unless
 * rows >= 1, 1 <= S <= rows (S == rows when seg_indptr is NULL), capacity >= 1, 0 <= layer_idx < L and the widths are as above;
 * ATOM_ERR_ALIGN unless y, x, the weights and t are 16-byte and the tables 4-byte aligned.
 *
 * atom_kv_quant_u4_f16: k fp16 [T, kv_heads, 128] -> packed u8 [T, kv_heads, 64] + param fp16 [T, kv_heads, 2] (scale, zero): the
 * per-head u4 quantiser of atom_kv_quant_append_f32 (the same device function) on float(k), written to plain tensors in the form
 * atom_kv_append_i4 takes -- for k / v that get an adapter's delta added before they are quantised.  head_dim must be 128;
 * ATOM_ERR_SHAPE unless T >= 1, kv_heads >= 1; ATOM_ERR_ALIGN unless k and packed are 16-byte and param 4-byte aligned.
 */
int atom_bgmv_f16(void *y, const void *x, const void *w, const int32_t *seg_adapter, const int32_t *seg_indptr, int64_t rows, int64_t S,
                  int64_t H1, int64_t H2, int64_t capacity, int64_t L, int64_t layer_idx, float scale, void *stream);
int atom_add_lora_f16(void *y, const void *x, const void *wa, const void *wb, const int32_t *seg_adapter, const int32_t *seg_indptr,
                      void *t, int64_t rows, int64_t S, int64_t H1, int64_t H2, int64_t rank, int64_t capacity, int64_t L,
                      int64_t layer_idx, float scale, void *stream);
int atom_kv_quant_u4_f16(const void *k, void *packed, void *param, int64_t T, int kv_heads, int head_dim, void *stream);

/*
 * Sampling: one token per row of fp16 logits under temperature, top-k and top-p -- csrc/sample.hip, arithmetic in csrc/sample_math.h,
 * the contract in DESIGN.md 4.13.  No reference counterpart (the reference's serving loop takes the argmax on the host).
 *   logits fp16 [batch, vocab], row stride ld >= vocab elements; tokens int64 [batch]
 *   temperature float [batch], top_k int32 [batch], top_p float [batch], seeds uint64 [batch], step int64 [1]: DEVICE arrays, read by
 *   the launch (a captured launch follows buffers that are changed in place); each may be NULL: T = 1, k off, p off, seed 0, *step = 0.
 * tokens[b] is a pure function of row b's bits, its four parameters and s = *step + step_offset -- not of the batch, the grid or the
 * order of any atomic:
 *   1. l_i = float(logit_i), NaN -> -inf, +inf -> 65504, -0 = +0; m = max l_i; m = -inf: token 0.
 *   2. order: l_i descending, the lower index first among equal logits.
 *   3. T <= 0 or NaN: the first token of the order (greedy).  Otherwise T is clamped to [2^-10, 2^10].
 *   4. w_i, 2^40 fixed point, FP32 with one rounding per operation: r = 1 / T, x = ((l_i - m) * r) * 0x1.715476p+0f; x < -40: w_i = 0;
 *      else n = floor(x), f = x - n, q = 2^f by the degree-5 Horner polynomial of sample_math.h, w_i = (uint64)(q * 2^23) << (17 + n)
 *      (a right shift where 17 + n < 0).  The maximum's weight is exactly 2^40.
 *   5. 0 < k < vocab: keep the first k of the order (else all); Z_k = their weight sum.
 *   6. p < 1 (or NaN): P = (uint64)(p * 2^32) (0 for p <= 0 or NaN), thr = (Z_k * P) >> 32; keep the shortest non-empty prefix whose
 *      weight sum is >= thr; Z = its sum.
 *   7. R = word 0 of Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (s & 0xffffffff, s >> 32, 0, 0); target = (Z * R) >> 32;
 *      the token is the first of the kept prefix whose cumulative weight is greater than target.
 * One launch, no workspace, nothing read back: capturable.  An index outside 0 .. vocab - 1 is never produced.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null logits / tokens; ATOM_ERR_SHAPE for batch < 1, vocab < 1,
 * vocab > 262144 or ld < vocab; ATOM_ERR_ALIGN for a pointer off its element size (2 bytes for logits, 4 for temperature / top_k /
 * top_p, 8 for seeds / step / tokens).  Rows whose base is 16-byte aligned with ld % 8 == 0 are read with 16-byte loads.
 */
int atom_sample_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const float *temperature, const int32_t *top_k,
                    const float *top_p, const uint64_t *seeds, const int64_t *step, int64_t step_offset, int64_t *tokens, void *stream);

/* The same with a draw number per sequence (the verify rows of speculative decoding): the `batch` rows are batch / rows_per_seq
 * sequences of rows_per_seq consecutive rows, step is int64 [batch / rows_per_seq], and row r draws number
 * s = step[r / rows_per_seq] + r % rows_per_seq + step_offset.  Everything else -- the per-ROW parameter arrays, the arithmetic, the
 * kernel -- is atom_sample_f16's.  Errors: as above, with ATOM_ERR_INVALID_ARG for a null step and ATOM_ERR_SHAPE for rows_per_seq < 1
 * or a batch that is not a multiple of it. */
int atom_sample_rows_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const float *temperature, const int32_t *top_k,
                         const float *top_p, const uint64_t *seeds, const int64_t *step, int64_t rows_per_seq, int64_t step_offset,
                         int64_t *tokens, void *stream);

/*
 * Token log-probabilities: per row of fp16 logits, the log-probability and rank of a target token and the top-n tokens with their
 * log-probabilities -- csrc/logprob.hip, on the sampler's arithmetic (csrc/sample_math.h), the contract in DESIGN.md 4.14.  What it
 * reports is the distribution atom_sample_f16 draws from at T = 1 without truncation.
 *   logits fp16 [rows, vocab], row stride ld >= vocab elements; targets int64 [rows] or NULL; logprob float [rows] or NULL;
 *   rank int32 [rows] or NULL; top_ids int64 / top_logprobs float [rows, top_n], required exactly when top_n >= 1; 0 <= top_n <= 32.
 * A row's result is a pure function of the row's bits and its target -- not of the grid, the batch or the order of any atomic:
 *   1. l_i, the order (l_i descending, lower index first) and m = max l_i as steps 1 - 2 of atom_sample_f16.
 *   2. w_i = the sampler's weight of l_i under m at T = 1 (never the sampler's temperature); Z = SUM w_i, an exact integer, 2^40 <= Z < 2^59.
 *   3. lz = (float)(log((double)Z) - 40 ln 2): Z converted round-to-nearest, log in double precision (sample_math.h log_z).
 *   4. lp_i = (l_i - m) - lz, two FP32 operations, one rounding each; l_i = -inf gives -inf.
 *   5. targets[r] = t in 0 .. vocab - 1: logprob[r] = lp_t, rank[r] = #{i : l_i > l_t} + #{i < t : l_i = l_t}, the 0-based position in
 *      the order (the greedy token has rank 0).
 *   6. any other t (negative, >= vocab): logprob[r] = 0, rank[r] = -1 (a loss's ignore_index); t is compared, never used as an address.
 *   7. top_ids[r, j], top_logprobs[r, j], j < top_n: the first top_n tokens of the order, in that order, with their lp; entries
 *      j >= vocab hold -1 and -inf.
 *   8. a row of -inf only (m = -inf): every lp is -inf, rank = t for a target in range, top_ids are 0, 1, ...
 * targets == NULL: logprob and rank are ignored, only the top-n is written.  The only inexact step is the double-precision log: a
 * host's libm may differ from the device's in the last double bit, so after the rounding to float the kernel's lz is a checker's lz
 * or a float32 neighbour of it.  One launch, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null logits, top_n >= 1 with a null top array, or nothing to do
 * (top_n = 0 and no targets, or both logprob and rank null); ATOM_ERR_SHAPE for rows < 1, vocab < 1, vocab > 262144, ld < vocab or
 * top_n outside 0 .. 32; ATOM_ERR_ALIGN for a pointer off its element size (2 bytes for logits, 4 for logprob / rank / top_logprobs,
 * 8 for targets / top_ids).  Rows whose base is 16-byte aligned with ld % 8 == 0 are read with 16-byte loads.
 */
int atom_logprob_f16(const void *logits, int64_t ld, int64_t rows, int64_t vocab, const int64_t *targets, float *logprob, int32_t *rank,
                     int64_t top_n, int64_t *top_ids, float *top_logprobs, void *stream);

/*
 * Logit penalties: repetition, presence and frequency penalties and a per-row logit bias on fp16 logits, with the occurrence state
 * advanced in the same launch -- csrc/penalize.hip, arithmetic in csrc/penalty_math.h, the contract in DESIGN.md 4.15.  No reference
 * counterpart.  The output feeds atom_sample_f16.
 *   logits fp16 [batch, vocab], row stride ld >= vocab; out fp16 [batch, vocab], row stride out_ld >= vocab.  out may equal logits
 *   (in place, then out_ld == ld); otherwise the two must not overlap.
 *   state int16 [batch, state_ld >= vocab] or NULL: one word per (sequence, token).  The sign bit: the token occurs in the prompt.  The
 *   low 15 bits: count, how often the token was fed back as a generated token, saturating at 32767.  NULL: nothing is seen, every
 *   count is 0 (fed must be NULL too).
 *   fed int64 [batch] or NULL; rep, pres, freq float [batch] or NULL (neutral: 1, 0, 0); bias_ids int32 [batch, max_bias] padded with
 *   -1 and bias_vals float [batch, max_bias], 0 <= max_bias <= 512 (both may be NULL when max_bias == 0).  All DEVICE arrays, read by
 *   the launch: a captured launch follows buffers that are changed in place.
 * Row b:
 *   1. Counting comes first: with fed given and 0 <= fed[b] < vocab, the count of state[b, fed[b]] is incremented (saturating, the
 *      sign bit kept) BEFORE the row is penalised, whatever the row's parameters are.  Any other fed[b] counts nothing; fed is
 *      compared with element positions, never used as an address.
 *   2. rep is off (treated as 1) when !(rep > 0); otherwise it is clamped to [2^-10, 2^10].  The row is NEUTRAL when rep is off or 1,
 *      pres == 0, freq == 0 and no bias entry of the row has an id >= 0: every 16-bit word of a neutral row is copied unchanged.
 *   3. seen = the sign bit is set or count > 0.  In a non-neutral row an element that is not seen and has no bias entry is copied
 *      bit for bit (NaN payloads, -0).
 *   4. Every other element, in FP32 with one rounding per line:
 *        l = (float)logit
 *        seen and rep on:  l = l > 0 ? l / rep : l * rep
 *        l = l - freq * (float)count              (the product, then the difference)
 *        count > 0:        l = l - pres
 *        bias entry:       l = l + bias
 *        out = (fp16)l, round to nearest even
 *      NaN, +-inf and a -inf bias follow IEEE; a computed NaN is written as 0x7E00 (IEEE leaves the payload open).  The prompt flag
 *      triggers the repetition penalty only: presence and frequency see generated tokens (the vLLM / OpenAI meaning).
 *   5. A bias id that is -1 (padding), negative or >= vocab is ignored.  Duplicate ids in one row are the caller's error: the result is
 *      then one of the addition orders, and stays in bounds.
 * One launch, a grid of (2048-element tile, row) workgroups, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null logits / out, fed without state, or max_bias > 0 with a null bias
 * array; ATOM_ERR_SHAPE for batch < 1, batch > 65535, vocab < 1, vocab > 262144, ld / out_ld / state_ld < vocab, max_bias outside
 * 0 .. 512, or out == logits with out_ld != ld; ATOM_ERR_ALIGN for a pointer off its element size (2 bytes for logits / out / state,
 * 4 for rep / pres / freq / bias_ids / bias_vals, 8 for fed).  When logits, out and state are 16-byte aligned with leading dimensions
 * that are multiples of 8, they are accessed 16 bytes at a time.
 */
int atom_penalize_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, int16_t *state, int64_t state_ld, const int64_t *fed,
                      const float *rep, const float *pres, const float *freq, const int32_t *bias_ids, const float *bias_vals,
                      int64_t max_bias, void *out, int64_t out_ld, void *stream);

/*
 * The same penalties on the verify rows of speculative decoding -- csrc/penalize.hip, the arithmetic of csrc/penalty_math.h unchanged,
 * the contract in DESIGN.md 4.20.  No reference counterpart.  A verify step scores rows = K + 1 rows per sequence; row j is penalised as
 * if drafts 1 .. j had been emitted, rejected drafts leave no trace, and the tokens the step before emitted are counted first.
 *   logits fp16 [batch * rows, vocab], rows ld apart (row b * rows + j is row j of sequence b); out likewise, out_ld apart; out may
 *   equal logits (then out_ld == ld).  state int16 [batch, state_ld >= vocab]: one row per SEQUENCE, the words of atom_penalize_f16.
 *   input_ids int64 [batch, rows], ids_ld apart: column 0 is the last emitted token, columns 1 .. rows - 1 the drafts.
 *   commit_tokens int64 [batch, >= commit_ld], commit_ld apart, and commit_counts int32 [batch]: the tokens to count first; both NULL:
 *   none.  rep, pres, freq float [batch] or NULL and bias_ids / bias_vals [batch, max_bias]: per SEQUENCE, as atom_penalize_f16 reads
 *   them per row.  All DEVICE arrays, read by the launch: a captured launch follows buffers that are changed in place.
 * Sequence b:
 *   1. Commit: c = commit_counts[b] clamped to 0 .. min(commit_ld, 9).  For i = 0 .. c - 1 in order, a commit_tokens[b][i] inside
 *      0 .. vocab - 1 has its state word counted up (saturating, the sign bit kept), once per occurrence: duplicates count twice.
 *      Any other value counts nothing.  Only these words of state are written, each only if it changes, whatever the sequence's
 *      parameters are.
 *   2. Rows: w_0 is the committed state row; for j >= 1, w_j is w_(j-1) with the word of input_ids[b][j] counted up, if that draft lies
 *      inside 0 .. vocab - 1.  Column 0 is NOT counted here: the step that emitted it committed it.  Drafts never reach state.
 *   3. Row (b, j) of out is, bit for bit, what atom_penalize_f16 writes for that row of logits under a state row w_j with fed = NULL and
 *      the parameters and bias list of sequence b: the neutral copy, the copy of what is neither seen nor biased, 0x7E00 for a
 *      computed NaN.
 *   4. logits == NULL and out == NULL: rule 1 alone (rows, input_ids, the parameters and the bias list are not read).
 *   Pending tokens, drafts and bias ids are compared with element positions, never used as addresses.
 * One launch, a grid of (2048-element tile, sequence) workgroups: the workgroup is the only one that touches its tile of the state, which
 * it reads once.  No workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for exactly one of logits / out null, exactly one of commit_tokens /
 * commit_counts null, nothing to do (neither logits nor pending tokens), a null state, a null input_ids when logits are given, or
 * max_bias > 0 with a null bias array; ATOM_ERR_SHAPE for batch outside 1 .. 65535, rows outside 1 .. 9, batch * rows beyond int32, vocab
 * outside 1 .. 262144, state_ld < vocab, commit_ld < 1 with pending tokens, max_bias outside 0 .. 512 and, when logits are given, ld /
 * out_ld < vocab, ids_ld < rows, or out == logits with out_ld != ld; ATOM_ERR_ALIGN for a pointer off its element size (2 bytes for
 * logits / out / state, 4 for commit_counts / rep / pres / freq / bias_ids / bias_vals, 8 for input_ids / commit_tokens).  When logits,
 * out and state are 16-byte aligned with leading dimensions that are multiples of 8, they are accessed 16 bytes at a time.
 */
int atom_penalize_rows_f16(const void *logits, int64_t ld, int64_t batch, int64_t rows, int64_t vocab, int16_t *state, int64_t state_ld,
                           const int64_t *input_ids, int64_t ids_ld, const int64_t *commit_tokens, int64_t commit_ld,
                           const int32_t *commit_counts, const float *rep, const float *pres, const float *freq, const int32_t *bias_ids,
                           const float *bias_vals, int64_t max_bias, void *out, int64_t out_ld, void *stream);

/*
 * Beam search, the selection step: per prompt group, the next w_out beams out of the candidates of its w_in rows -- csrc/beam.hip,
 * arithmetic in csrc/beam_math.h, the contract in DESIGN.md 4.16.  No reference counterpart.  The candidates are the top-n of
 * atom_logprob_f16: the best w_out of all w_in x vocab continuations lie within the union of each row's best w_out.
 *   top_ids int64 / top_lp float [groups * w_in, C]: row b's C most probable tokens and their log-probabilities, in its order;
 *   cum float, finished int32 (0 / non-zero), length int32 [groups * w_in]: each row's sum of log-probabilities, whether it has ended
 *   and how many tokens it holds; eos: the token that ends a hypothesis, negative for none.
 *   parent int32 (the row INSIDE the group, 0 .. w_in - 1), token int64, cum_out float, finished_out int32, length_out int32
 *   [groups * w_out].  An output may be the input of the same name when w_in == w_out; otherwise the arrays must not overlap.
 *   1 <= w_out <= 16; w_in is 1 (the step after the prefill) or w_out; w_out <= C <= 32.
 * Group g, rows b = 0 .. w_in - 1:
 *   1. A live row (finished == 0) has the candidates (b, c), c = 0 .. C - 1, with score s = cum[b] + top_lp[b][c]: ONE FP32 addition.
 *   2. A finished row has exactly one candidate, (b, 0), with score cum[b]: the hypothesis is frozen and competes by its final sum.
 *      Nothing is normalised by length during the search.
 *   3. Scores are compared through a 32-bit key: u = the score's bits; -0 -> +0; NaN -> -inf; key = u & 0x80000000 ? ~u : u | 0x80000000.
 *      A larger key is a larger score; -inf has the smallest key.  No NaN arises from clean inputs: a log-probability is never +inf,
 *      hence neither is a sum of them, and -inf + lp is -inf.
 *   4. The winners are the first w_out candidates of the total order: key descending, then b ascending, then c ascending
 *      (atom_logprob_f16 already orders equal log-probabilities by token id).  Output i of the group is the i-th of them.
 *   5. A winner (b, c) of a live row: parent = b, token = top_ids[b][c], cum_out = s, length_out = length[b] + 1,
 *      finished_out = (eos >= 0 and token == eos).
 *   6. The winner of a finished row: parent = b, token = max(eos, 0), cum_out = cum[b], length_out = length[b], finished_out = 1.
 *   7. Fewer than w_out candidates (only w_in == 1 with a finished row): the remaining outputs are parent 0, token max(eos, 0),
 *      cum_out -inf, finished_out 1, length_out = length[0].
 * Token ids pass through unchanged: they are never used as an address here.  One launch of `groups` workgroups, no workspace, nothing
 * read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer; ATOM_ERR_SHAPE for groups < 1, w_out outside 1 .. 16,
 * w_in neither 1 nor w_out, C < w_out or C > 32; ATOM_ERR_ALIGN for a pointer off its element size (8 bytes for top_ids / token, 4 for
 * the others).
 */
int atom_beam_select(const int64_t *top_ids, const float *top_lp, const float *cum, const int32_t *finished, const int32_t *length,
                     int64_t groups, int w_in, int w_out, int C, int64_t eos, int32_t *parent, int64_t *token, float *cum_out,
                     int32_t *finished_out, int32_t *length_out, void *stream);

/*
 * Beam search, the cache step: the rows of a static INT4 paged cache (the buffers of atom_kv_step_i4) reordered by `parent`, on the
 * device -- csrc/beam.hip, DESIGN.md 4.16.  Row r of group r / w continues the history of row p = (r / w) * w + parent[r].
 *   kv_data / kv_param: the pool (layout above), `capacity` pages; both 16-byte aligned.
 *   table_in int32 [batch, cap], spare_in int32 [batch]: the page tables and one page per row that no table references (read only);
 *   table_out, spare_out: what the launch writes; they must not overlap table_in / spare_in (rows are read by other rows'
 *   workgroups).  The caller copies them back, device to device on the same stream.
 *   row_pages, lens, state: as atom_kv_step_i4; the lengths are READ at the current parity (state[1] & 1) and not written.
 *   parent int32 [batch], each in 0 .. w - 1; batch is a multiple of w, 1 <= w <= 16.
 * All rows of a group hold the same number of tokens L (the invariant of beam search).  With full = L / page_size, off = L % page_size:
 *   j < full             table_out[r][j] = table_in[p][j]: full pages are immutable and shared by reference.
 *   j == full, off > 0   p == r: table_in[r][j].  Otherwise page table_in[p][j] is copied whole (both pool buffers: all layers, K and V,
 *                        all heads; 16-byte loads and stores) into page spare_in[r]; table_out[r][j] = spare_in[r] and
 *                        spare_out[r] = table_in[r][j].  (Else spare_out[r] = spare_in[r].)
 *   later j              table_out[r][j] = table_in[r][j]: the row's own untouched reserve.
 * So no partial page is ever referenced by two rows, and the page a row writes is never one another row reads in the same launch.
 * A parent outside 0 .. w - 1 keeps the row as it is and sets ATOM_KV_BEAM_BAD_PARENT in state[0]; a length outside the row's reserve
 * is clamped and sets ATOM_KV_STEP_BAD_LENGTH; a page id outside 0 .. capacity - 1 where a copy is due keeps the row and sets
 * ATOM_KV_BEAM_BAD_PAGE -- it is never used as an address.  Every id written is one read from table_in or spare_in.
 * One launch, nothing read back: capturable.
 * Errors: ATOM_ERR_INVALID_ARG for a null pointer or table_out / spare_out overlapping table_in / spare_in; ATOM_ERR_SHAPE for the
 * cache's shape (head_dim != 128, page_size not a multiple of 16, ...), w outside 1 .. 16, batch not a multiple of w, cap < 1,
 * capacity < 1, cap * page_size or batch * cap beyond int32; ATOM_ERR_ALIGN for kv_data / kv_param off 16 bytes or a table off 4.
 */
#define ATOM_KV_BEAM_BAD_PARENT 4
#define ATOM_KV_BEAM_BAD_PAGE 8
int atom_kv_beam_fork_i4(void *kv_data, void *kv_param, const int32_t *table_in, int32_t *table_out, const int32_t *spare_in,
                         int32_t *spare_out, const int32_t *row_pages, const int32_t *lens, int32_t *state, const int32_t *parent,
                         int batch, int w, int cap, int64_t capacity, int num_layers, int num_heads, int page_size, int head_dim,
                         void *stream);

/*
 * Speculative decoding, the drafter: K guessed tokens per sequence by n-gram lookup in the sequence's own history (prompt-lookup
 * decoding) -- csrc/spec.hip, the integer rules in csrc/spec_math.h, DESIGN.md 4.17.
 *   hist int32 [batch, hist_cap]: the prompt and every emitted token; hist_len int32 [batch]
 *   1 <= ngram_min <= ngram_max <= 8; 1 <= K <= 8
 *   out int64, row b at out + b * out_ld (out_ld >= K elements): the drafts land directly in columns 1 .. K of the verify step's
 *   input_ids [batch, K + 1] (out = input_ids + 1, out_ld = K + 1); nothing else of a row is written.
 * One row, len = hist_len[b]:
 *   1. For n = ngram_max down to ngram_min, skipping every n with len <= n:
 *   2. among the starts s with 0 <= s and s + n <= len - 1 keep those with hist[s .. s+n) == hist[len-n .. len);
 *   3. take the largest such s (the most recent occurrence); 4. the first n that has one wins.
 *   5. Draft j (0 .. K - 1) is hist[s + n + j] if s + n + j < len, otherwise hist[len - 1].
 *   6. With no occurrence at any n, all K drafts are hist[len - 1].
 * A row with len <= 0 or len > hist_cap gets K drafts of token 0 and nothing of it is read.  No index outside 0 .. len - 1 of the row
 * is ever read.  One launch of `batch` workgroups, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer; ATOM_ERR_SHAPE for batch < 1, hist_cap < 1 (either
 * beyond int32), K or the n-gram sizes outside the ranges above, out_ld < K; ATOM_ERR_ALIGN for hist / hist_len off 4 bytes, out off 8.
 */
int atom_spec_draft_ngram(const int32_t *hist, const int32_t *hist_len, int64_t batch, int64_t hist_cap, int ngram_min, int ngram_max,
                          int K, int64_t *out, int64_t out_ld, void *stream);

/*
 * Speculative decoding, accept and commit: compares the drafts with the tokens chosen at the verify rows, emits the agreed prefix
 * plus the model's own next token and prepares the next step -- csrc/spec.hip, DESIGN.md 4.17.  Q = K + 1, 1 <= K <= 8.
 *   targets   int64 [batch, Q]   the token chosen at every verify row (read only)
 *   input_ids int64 [batch, Q]   column 0 the last emitted token, columns 1 .. K the drafts
 *   n_out int32 [batch] tokens emitted so far; budget int32 [batch] (read only)
 *   tokens int64 [batch, max_new]; hist int32 [batch, hist_cap], hist_len int32 [batch]
 *   adds int32 [batch], draw int64 [batch], accepted int32 [batch], steps int32 [batch], done int32 [1]
 * Row b: a = the number of leading j < K with input_ids[b][1 + j] == targets[b][j]; e = min(a + 1, max(budget[b] - n_out[b], 0)).
 *   tokens[b][n_out .. n_out + e) = targets[b][0 .. e), the same e tokens go to hist[b] at hist_len[b]; a position outside
 *   0 .. max_new - 1 (0 .. hist_cap - 1) is skipped, whatever the buffers hold.
 *   adds[b] = e (what the next atom_kv_step_rows_i4 commits).  With e > 0: n_out[b] += e, hist_len[b] += e,
 *   input_ids[b][0] = targets[b][e - 1], draw[b] = the new n_out[b] (the sampler's next draw base), accepted[b] += e - 1, steps[b] += 1.
 *   With e = 0 (a row at its budget) nothing but adds[b] = 0 is written.
 *   done[0] = 1 if every row has n_out >= budget after this launch, else 0: computed from all rows inside the launch.
 * A row's targets and drafts are read before anything of the row is written.  One launch of one workgroup, no workspace, nothing
 * read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer; ATOM_ERR_SHAPE for batch < 1, K outside 1 .. 8,
 * max_new < 1, hist_cap < 1 (each beyond int32 too); ATOM_ERR_ALIGN for a pointer off its element size.
 */
int atom_spec_accept(const int64_t *targets, int64_t *input_ids, int32_t *n_out, const int32_t *budget, int64_t *tokens, int32_t *hist,
                     int32_t *hist_len, int32_t *adds, int64_t *draw, int32_t *accepted, int32_t *steps, int32_t *done, int64_t batch,
                     int K, int64_t max_new, int64_t hist_cap, void *stream);

/*
 * Guided decoding: which tokens a sequence may emit next, as a function of what it has emitted -- a deterministic automaton over token
 * ids, its allowed sets applied to the logits and its states stepped on the device -- csrc/guide.hip, rules in csrc/guide_math.h, the
 * contract in DESIGN.md 4.18.  No reference counterpart.  The masked row feeds atom_sample_f16 (which never draws -inf) or an argmax.
 * The automaton has num_states states; several automata serve one batch stacked into one table, a state being a global index.
 *   edges, CSR: indptr int32 [num_states + 1]; edge_tok int32 [num_edges], strictly ascending inside indptr[s] .. indptr[s + 1];
 *   edge_next int32 [num_edges], the state the edge leads to.
 *   mask uint32 [num_states, mask_ld], mask_ld >= ceil(vocab / 32): token v is allowed in state s iff
 *   (mask[s * mask_ld + (v >> 5)] >> (v & 31)) & 1.  The caller derives it from the edges.
 *   state int32 [batch]: a state, ATOM_GUIDE_FREE (unconstrained) or ATOM_GUIDE_DEAD (the sequence left its language: unconstrained
 *   from then on).  status int32 [1]: the launches only ever set bits in it.
 *   All DEVICE arrays, read by the launch: a captured launch follows buffers that are changed in place.
 */
#define ATOM_GUIDE_FREE (-1)
#define ATOM_GUIDE_DEAD (-2)
#define ATOM_GUIDE_REJECTED 1
#define ATOM_GUIDE_BAD_STATE 2
/*
 * The mask.  logits fp16 [batch, vocab], row stride ld >= vocab; out fp16 [batch, vocab], row stride out_ld >= vocab.  out may equal
 * logits (in place, then out_ld == ld); otherwise the two must not overlap.  Row b, s = state[b]:
 *   1. 0 <= s < num_states: out[b, v] is logits[b, v] bit for bit (NaN payloads, -0) where v is allowed in s, 0xFC00 (-inf) elsewhere.
 *   2. s == ATOM_GUIDE_FREE or ATOM_GUIDE_DEAD: the row is copied bit for bit.
 *   3. Any other s: the row is copied and ATOM_GUIDE_BAD_STATE is set.  s is compared before it is ever used as an index.
 *   4. Columns vocab .. out_ld - 1 are never written; mask bits at positions >= vocab and mask words >= ceil(vocab / 32) of a row are
 *      never looked at.
 *   5. The result is a function of the row, its state and its mask row alone, whatever the grid and the batch.
 * One launch, a grid of (2048-element tile, row) workgroups, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer; ATOM_ERR_SHAPE for batch < 1, batch > 65535, vocab < 1,
 * vocab > 262144, ld / out_ld / 32 * mask_ld < vocab, num_states < 1, num_states * mask_ld beyond int32, or out == logits with
 * out_ld != ld; ATOM_ERR_ALIGN for a pointer off its element size (2 bytes for logits / out, 4 for state / mask / status).  When logits
 * and out are 16-byte aligned with leading dimensions that are multiples of 8, they are accessed 16 bytes at a time; the mask is read by
 * the byte (the eight bits of a thread's eight elements) and needs no more than its element's alignment.
 */
int atom_guide_mask_f16(const void *logits, int64_t ld, int64_t batch, int64_t vocab, const int32_t *state, const uint32_t *mask,
                        int64_t mask_ld, int64_t num_states, void *out, int64_t out_ld, int32_t *status, void *stream);

/*
 * The step.  tokens int64 [batch]: the token every sequence has just emitted.  Sequence b, s = state[b], t = tokens[b] (compared as
 * int64: 2^32 + 5 does not match edge token 5):
 *   1. s == ATOM_GUIDE_FREE stays FREE, s == ATOM_GUIDE_DEAD stays DEAD.
 *   2. 0 <= s < num_states: lo = indptr[s], hi = indptr[s + 1], both clamped into 0 .. num_edges, hi raised to lo if below it; t is
 *      looked up in edge_tok[lo .. hi) by binary search.
 *        found at e, 0 <= edge_next[e] < num_states:   state[b] = edge_next[e]
 *        found at e, edge_next[e] outside that range:  state[b] = ATOM_GUIDE_DEAD, ATOM_GUIDE_BAD_STATE is set
 *        not found (an empty range included):          state[b] = ATOM_GUIDE_DEAD, ATOM_GUIDE_REJECTED is set
 *   3. Any other s: state[b] = ATOM_GUIDE_DEAD, ATOM_GUIDE_BAD_STATE is set.
 * One thread per sequence, state updated in place.  No index outside its checked range is dereferenced: a bad table or token is a
 * status bit, never a fault.  (Edge tokens that are not ascending make the search miss edges; they cannot make it leave the range.)
 * One launch, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer (edge_tok / edge_next may be null when num_edges == 0);
 * ATOM_ERR_SHAPE for batch < 1, batch > 65535, num_states < 1, num_edges < 0, either beyond int32; ATOM_ERR_ALIGN for a pointer off
 * its element size (8 bytes for tokens, 4 for the others).
 */
int atom_guide_advance(int32_t *state, const int64_t *tokens, int64_t batch, const int32_t *indptr, const int32_t *edge_tok,
                       const int32_t *edge_next, int64_t num_states, int64_t num_edges, int32_t *status, void *stream);

/*
 * The verify rows of a guided speculative step: the automaton state behind each of a sequence's rows = Q = K + 1 input
 * tokens, the commit of the step before folded in, and drafts that a state forces written over what the drafter proposed.
 *   state int32 [batch]: the committed state, the one BEFORE input_ids[b][0].  adds int32 [batch]: the rows the last step committed
 *   (atom_spec_accept's adds; 0 before the first step).  row_state int32 [batch, rows], contiguous: on entry the last step's row
 *   states, on return this step's.  input_ids int64 [batch, rows], row stride ids_ld >= rows: column 0 the last emitted token, columns
 *   1 .. rows - 1 the drafts.  force: 0 leaves every draft as it is.
 * Sequence b, a = adds[b]:
 *   1. Commit.  s = row_state[b][a - 1] if 1 <= a <= rows; s = state[b] if a == 0; any other a: s = state[b] and
 *      ATOM_GUIDE_BAD_STATE is set.  If state[b] != ATOM_GUIDE_DEAD and s == ATOM_GUIDE_DEAD, ATOM_GUIDE_REJECTED is set: a token
 *      without an edge has been emitted.  This is the only place the entry sets that bit.  state[b] = s (written only if it differs).
 *   2. Walk.  r = s; for j = 0 .. rows - 1:
 *        a. if force, j >= 1, 0 <= r < num_states and the range indptr[r] .. indptr[r + 1] (clamped as atom_guide_advance clamps it)
 *           holds exactly one edge e: input_ids[b][j] = edge_tok[e].  No other element of input_ids is written.
 *        b. r = the state atom_guide_advance gives for (r, input_ids[b][j]), except that a token without an edge gives
 *           ATOM_GUIDE_DEAD and sets NO bit: a wrong draft is not an error, its rows are discarded by atom_spec_accept.  FREE and DEAD
 *           stay; a state or an edge target outside the table gives DEAD and ATOM_GUIDE_BAD_STATE.
 *        c. row_state[b][j] = r: row j's logits predict the token after input_ids[b][j], so r is the state atom_guide_mask_f16 masks
 *           that row with (its state argument is row_state, one state per row of the batch * rows logit rows).
 *   3. input_ids == NULL is the commit alone (after the last step): rule 1 runs, row_state is left as it is.
 * One thread per sequence; a thread reads and writes its own sequence's elements only, and reads row_state[b][a - 1] before it writes
 * the row, so folding the commit of step n into the walk of step n + 1 needs no second buffer.  No index outside its checked range is
 * dereferenced.  One launch, no workspace, nothing read back: capturable.
 * Errors (checked before the launch): ATOM_ERR_INVALID_ARG for a null pointer (input_ids may be null; edge_tok / edge_next may be null
 * when num_edges == 0); ATOM_ERR_SHAPE for batch < 1, batch > 65535, rows < 1, rows > 9, ids_ld < rows, num_states < 1,
 * num_edges < 0, either beyond int32; ATOM_ERR_ALIGN for a pointer off its element size (8 bytes for input_ids, 4 for the others).
 */
int atom_guide_walk_rows(int32_t *state, const int32_t *adds, int32_t *row_state, int64_t *input_ids, int64_t ids_ld, int64_t batch,
                         int64_t rows, const int32_t *indptr, const int32_t *edge_tok, const int32_t *edge_next, int64_t num_states,
                         int64_t num_edges, int32_t force, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ATOM_HIP_H_ */
