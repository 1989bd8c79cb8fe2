/*
 * fastvocoder_hip.h -- C ABI of libfastvocoder_hip.so, the MI355X (gfx950)
 * replacement for the ATen calls on FastVocoder's generator forward path.
 *
 * The reference has no FFI on this path: its generators are torch.nn.Modules
 * whose arithmetic is delegated to ATen.  Each entry
 * point below names the reference call site(s) whose arithmetic it replaces
 * (paths relative to /root/reference).  The Python host side
 * (the fastvocoder_amd/generator package) mirrors the reference's module API and is
 * the only caller; INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer to
 *     contiguous fp32 in the reference's [B, C, T] layout unless stated;
 *   - the library owns no device memory: callers pass inputs, outputs, packed
 *     weights and workspace, and keep them alive until the stream has drained;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     every call only enqueues work on it and returns (no device sync);
 *   - return value: 0 on success, otherwise a hipError_t or FV_ERR_* code,
 *     with a thread-local message available from fv_last_error();
 *   - re-entrant per (device, stream): results depend on no process-wide state.  What the library keeps per process
 *     is host-side and either a cache of pure functions of a launch's shape, protected by a mutex (block schedules, tile
 *     width plans, the list of kernels granted a dynamic LDS size) or written once (the tuning table, the device's CU
 *     count); the error text is thread-local.  Calls from several threads, each on a stream and on module state of its
 *     own, need no lock (tests/test_gpu_threads.py).  fv_tuning_set, fv_profile_* and the launch log (fv_debug_launch_log)
 *     are process-wide hooks of tests and tools: not for concurrent use with each other or with themselves.
 */
#ifndef FASTVOCODER_HIP_H
#define FASTVOCODER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV_ABI_VERSION 18   /* 18: fv_stft_distance_grad (entries added since -- the latest: fv_debug_launch_log_streams -- change no existing one); 17: Griffin-Lim (fv_stft, fv_istft, fv_griffin_lim, ...) */
/* Entry points are added under one version number: 18 also covers the gradient, optimizer and training entries that
 * came after fv_stft_distance_grad, the latest being fv_conv1d_weight_grad_dilated_bf16 and
 * fv_conv_transpose1d_weight_grad_bf16 (the generators' bf16 weight gradients).  No existing entry changed its signature or its result. */

#define FV_ERR_INVALID_ARG (-1)
#define FV_ERR_UNSUPPORTED (-2)
#define FV_ERR_WORKSPACE (-3)
/* a split-f16 kernel met an operand beyond the f16 range or a non-finite value (fv_plan_check_range): the run's results
 * are not valid; the caller repeats it with FV_PAIR_F32 arithmetic */
#define FV_ERR_RANGE (-4)
/* ... the same for the LOW side of the domain only (operands that were smaller than 2^-10 throughout a block's share of a
 * tensor): the run's results may carry fewer than 22 bits; repeating THIS run with FV_PAIR_F32 is enough -- the condition is
 * a property of the input, not of the model */
#define FV_ERR_RANGE_LOW (-5)
/* the two sides of a `guard` word: separate BYTES of the int32, so that plain stores from different blocks and launches
 * combine (a store to one byte never takes back the other) */
#define FV_GUARD_HIGH 0x001
#define FV_GUARD_LOW 0x100

/* padding of a conv's input: zero "same" padding (torch.nn.Conv1d padding=,
 * model/generator/modules.py:193-221) or reflection padding + valid conv
 * (torch.nn.ReflectionPad1d, modules.py:355-356, melgan.py:68-71) */
#define FV_PAD_ZERO 0
#define FV_PAD_REFLECT 1
/* flag ORed into pad_mode: keep only the first Tin outputs (the reference's CausalConv1d,
 * modules.py:273-294: pad (k-1)*dil on BOTH sides with the configured pad module, valid
 * conv, then [:, :, :T]); pass pad = (k-1)*dil */
#define FV_PAD_CAUSAL 2

/* activation applied after the epilogue adds */
#define FV_POST_NONE 0
#define FV_POST_TANH 1 /* torch.tanh, hifigan.py:106 / melgan.py:108-109 */
#define FV_POST_RELU 2 /* torch.nn.ReLU, basis_melgan.py:120-121 */

int fv_version(void);
/* hash of the sources this binary was built from (fastvocoder_amd/_native.py source_hash()): lets a
 * test prove that the loaded library is the working tree's, not a stale prebuilt one */
const char* fv_build_id(void);
/* thread-local description of the last non-zero return on this thread */
const char* fv_last_error(void);

/* ------------------------------------------------------------------ *
 * one-off weight preparation (at load_state_dict / remove_weight_norm)
 * ------------------------------------------------------------------ */

/* torch.nn.utils.weight_norm reparametrisation w = v * g / ||v||_2, the norm
 * over every dim but 0 (hifigan.py:58-76; for ConvTranspose1d dim 0 is the
 * INPUT channel).  v, w: [dim0, inner]; g: [dim0]. */
int fv_fold_weight_norm(const float* v, const float* g, float* w, int dim0,
                        int64_t inner, void* stream);

/* Eval-mode BatchNorm1d folded into the 1x1/short conv that FOLLOWS it (LastLinear,
 * modules.py:116-132: act -> bn -> conv1x1):  conv(bn(x)) = conv'(x) with
 *   w'[co,ci,j] = w[co,ci,j] * a[ci],  b'[co] = b[co] + sum_{ci,j} w[co,ci,j] * c[ci],
 *   a = gamma / sqrt(var + eps),  c = beta - mean * a.
 * w [Cout,Cin,k]; b [Cout] or NULL (treated as 0); gamma/beta may be NULL (1 / 0);
 * w_out [Cout,Cin,k], b_out [Cout] (always written).  Exact only for valid / unpadded
 * convs (LastLinear's are 1x1). */
int fv_fold_batchnorm_conv(const float* w, const float* b, const float* gamma, const float* beta,
                           const float* mean, const float* var, float eps, float* w_out,
                           float* b_out, int Cout, int Cin, int k, void* stream);

/* Number of floats of the packed (K-major, M-padded) image of a Conv1d weight
 * [Cout, Cin, k] / of the polyphase image of a ConvTranspose1d weight
 * [Cin, Cout, k] with the given stride and padding. */
int64_t fv_packed_conv1d_floats(int Cout, int Cin, int k);
int64_t fv_packed_conv_transpose1d_floats(int Cin, int Cout, int k, int stride, int pad);

/* w [Cout, Cin, k] (torch.nn.Conv1d.weight) -> packed image */
int fv_pack_conv1d_weight(const float* w, float* packed, int Cout, int Cin, int k,
                          void* stream);
/* w [Cin, Cout, k] (torch.nn.ConvTranspose1d.weight) -> packed polyphase image */
int fv_pack_conv_transpose1d_weight(const float* w, float* packed, int Cin, int Cout,
                                    int k, int stride, int pad, void* stream);

/* ------------------------------------------------------------------ *
 * fused operators
 * ------------------------------------------------------------------ */

/*
 * y     = post( ( (acc_in + acc_in2) + ( conv1d(lrelu(x, pre_slope); w, dil, pad) + bias + res ) ) / out_div )
 * y_act = lrelu(y, act_slope)            (optional second output, see below)
 *
 * Replaces F.leaky_relu + torch.nn.Conv1d (+ the residual add, the MRF running
 * sum / mean and tanh) at modules.py:223-230 (ResBlock1), :247-252 (ResBlock2),
 * :372-382 (ResidualStack), :85-89 (LastLayer), hifigan.py:93,99-106,
 * multiband_hifigan.py:102-115, melgan.py:66-71.
 *   x [B,Cin,Tin]; packed from fv_pack_conv1d_weight; bias [Cout] or NULL;
 *   res, acc_in, acc_in2 [B,Cout,Tout] or NULL (acc_in + acc_in2 is formed first: the
 *   reference's xs = r0; xs += r1; xs += r2 order, hifigan.py:99-102); y [B,Cout,Tout],
 *   Tout = Tin + 2*pad - dil*(k-1) (Tin with FV_PAD_CAUSAL).  pre_slope = 1 disables the input
 *   activation, 0 is ReLU; out_div = 1 disables the division (it is a true
 *   fp32 division, hifigan.py:103).  y may alias res or acc_in, never x.
 *   Activation hoisting: plain VALU work does not overlap the fp32 MFMA on gfx950,
 *   so the fastest way to feed the NEXT conv's F.leaky_relu(x, s) is to have THIS
 *   conv store it.  With y_act != NULL the raw y (for residual consumers) and
 *   y_act = lrelu(y, act_slope) (for conv consumers, which then pass
 *   pre_slope = 1) are both written; with y_act == NULL and act_slope != 1 only
 *   the activated tensor is written, to y.  act_slope = 1 disables both.
 */
int fv_conv1d_fused(const float* x, const float* packed, const float* bias,
                    const float* res, const float* acc_in, const float* acc_in2, float* y,
                    float* y_act, int B, int Cin, int Cout, int Tin, int k, int dil, int pad,
                    int pad_mode, float pre_slope, float out_div, int post, float act_slope,
                    void* stream);

/*
 * Fused ResBlock1 pair (model/generator/modules.py:223-230, one iteration of the loop):
 *
 *     y_j = x_j + conv1d( lrelu( conv1d( lrelu(x_j, slope); w1_j, k_j taps, dilation dil ) + b1_j, slope ); w2_j, k_j taps ) + b2_j
 *
 * for n = 1..3 independent members j in ONE launch -- the pairs at the same position of the three
 * ResBlocks of an MRF stage (hifigan.py:97-103; taps 11 / 7 / 3, same dilation).  Both convs use 'same'
 * zero padding.  The intermediate tensor lives in LDS only; x_j is read raw (the activation is applied
 * on chip) and y_j is written raw, so no activated twin tensors exist between the pairs of a block.
 *   x_j, y_j [B,C,T]; w1_j, w2_j: fv_pack_pair_weight images of the [C,C,k_j] Conv1d weights;
 *   b1_j, b2_j [C] or NULL (the arrays themselves may be NULL); y_act (array or its entries may be
 *   NULL): optional second output lrelu(y_j, act_slope) for a conv1d consumer; with y_act[j] == NULL and
 *   act_slope != 1 only the activated tensor is written, to y_j.
 * Supported: C = 16 or 32, k_j in {3, 7, 11}, dil in {1, 3, 5}, T % 4 == 0 (rows 16-byte aligned);
 * anything else returns FV_ERR_UNSUPPORTED (use two fv_conv1d_fused calls).  Persistent blocks, each
 * with a contiguous cost-balanced share of the (member, utterance, tile) list; every output element is
 * computed the same way whichever block owns its tile: results do not depend on B or on how a batch is
 * split over calls.
 */
int64_t fv_packed_pair_floats(int C, int k);
/* w [C, C, k] (torch.nn.Conv1d.weight of a ResBlock conv) -> the A-fragment image the pair kernels read */
int fv_pack_pair_weight(const float* w, float* packed, int C, int k, void* stream);
int fv_resblock1_fused(int n, const float* const* x, const float* const* w1, const float* const* w2,
                       const float* const* b1, const float* const* b2, float* const* y, float* const* y_act,
                       const int* k, int B, int C, int T, int dil, float slope, float act_slope, void* stream);

/*
 * The same operator with a choice of arithmetic, and -- for the last launch of an MRF stage -- the merge
 * of hifigan.py:99-103 in the epilogue.
 *   prec = FV_PAIR_F32:       v_mfma_f32_16x16x4_f32, exact fp32 products (the functions above).
 *   prec = FV_PAIR_SPLIT_F16: every fp32 operand v is split as v = h1 + h2/2048 (+ <= 2^-22 |v|), h1, h2 f16,
 *       and a product is three v_mfma_f32_16x16x32_f16 terms a1 b1 + (a1 b2 + a2 b1)/2048 accumulated in
 *       fp32.  Per layer the result is as close to the exact sum as an fp32 FMA chain (measured: DESIGN.md
 *       section 3.7, tests/test_split_precision.py); 5.3x fewer matrix-core cycles, which turns the C = 16
 *       layers from matrix-bound into HBM / LDS-bound.  DOMAIN -- where the reference (fp32 ATen) is defined for any
 *       finite fp32 -- enforced, not assumed:
 *         weights: any finite fp32.  The pack functions scale every GEMM row by a power of two so that its largest
 *           magnitude lies in [2^13, 2^14) (exact; the f16 pair keeps 22 bits of every element down to 2^-28 of the
 *           row's maximum) and store the inverse behind the image; the kernels multiply the accumulated sum by it inside
 *           the fused multiply-add that adds the bias (exact).  `range_flag` is raised for a non-finite weight.
 *         activations, high side: |v| < 65520.  An operand beyond the f16 range turns into inf in f16 and every output
 *           it feeds into inf / NaN: every split-f16 kernel raises its `guard` word (FV_GUARD_HIGH: byte 0) when a final value is not
 *           finite.
 *         activations, low side: below 2^-14 the pair keeps an absolute 2^-36 instead of 22 bits -- harmless inside an
 *           ordinary tensor, a loss for one that is small as a whole (with correspondingly large weights behind it).
 *           Every kernel keeps the largest magnitude of the operands it splits; a block whose operands were not all zero
 *           and all below 2^-10 raises `guard` (FV_GUARD_LOW: byte 1; the two sides never overwrite each other).
 *         In both cases the caller repeats the layer / the run with FV_PAIR_F32 (fv_plan_check_range).
 *       range_flag / guard: int32 words any kernel can write (device memory or pinned host memory), NULL = no check.
 *       Weights: fv_pack_pair_weight_ex(prec) images ([K step][row half][split half][lane][8 f16], then one float per
 *       row: the inverse prescale).
 *       C = 16 / 32: one fused launch (intermediate and weights in LDS).  C = 64: one fused launch, the weights of
 *       both convs stream through an LDS ring (csrc/convp_kernels.hpp).  C = 128 / 256 / 512: the pair's two LDS images do not
 *       fit next to the ring; it runs as two launches of the split-f16 conv kernel (csrc/convh_kernels.hpp) and
 *       needs mid[j], a [B,C,T] scratch tensor per member (ignored at C = 64, NULL below).
 *   add1 / add2 (arrays or entries may be NULL; FV_PAIR_SPLIT_F16 only): member j stores
 *       y_j = post( ((x'_j + add1_j) + add2_j) / out_div )  -- with x'_j the first ResBlock's result and
 *       add1 / add2 the second and third this is xs = r0; xs += r1; xs += r2; x = xs / 3 in the
 *       reference's association.  Members without add1 ignore out_div / post.
 */
#define FV_PAIR_F32 0
#define FV_PAIR_SPLIT_F16 1
int64_t fv_packed_pair_floats_ex(int C, int k, int prec);
int fv_pack_pair_weight_ex(const float* w, float* packed, int C, int k, int prec, int* range_flag, void* stream);
int fv_resblock1_fused_ex(int n, const float* const* x, const float* const* w1, const float* const* w2,
                          const float* const* b1, const float* const* b2, float* const* y, float* const* y_act,
                          float* const* mid, const float* const* add1, const float* const* add2, const int* k, int B,
                          int C, int T, int dil, float slope, float out_div, int post, float act_slope, int prec,
                          int* guard, void* stream);

/*
 * A whole MRF stage of 16 channels as ONE launch (reference model/generator/hifigan.py:97-103 around
 * model/generator/modules.py:223-230), split-f16 operands (arithmetic and domain: FV_PAIR_SPLIT_F16 above):
 *
 *     r_j = ResBlock1_j(x),  j = 0, 1, 2:   three times  x <- x + conv1d( lrelu( conv1d( lrelu(x, slope); w1, k_j taps,
 *                                            dilation dil[p] ) + b1, slope ); w2, k_j taps ) + b2      (p = 0, 1, 2)
 *     y   = post( ((r_0 + r_1) + r_2) / out_div ),      y_act = lrelu(y, act_slope)
 *
 * -- the reference's association of the sum; every conv with 'same' zero padding.  What fv_resblock1_fused_ex computes in
 * four dependent launches per stage (three pair positions, the last one split for the merge), each of which reads and
 * writes the stage's tensor, is here one pass: a tile's columns stay on the CU through all 18 convs (running x in
 * registers, operand images and a few columns of history per conv in LDS, csrc/mrfh_kernels.hpp), x is read once and y
 * written once.  Bit-identical to the pair launches.
 *   x, y, y_act [B, C, T] (y_act or NULL; without it and act_slope != 1, y itself is stored activated); any T.
 *   k[3]: taps of the three ResBlocks, each 3, 7 or 11; dil[3] = {1, 3, 5}; C = 16 or 32.  Anything else: FV_ERR_UNSUPPORTED.
 *   C = 32 (csrc/mrfw_kernels.hpp: weights stream through LDS in pieces of four taps, the columns of history live in
 *   `workspace`): workspace = fv_mrf_stage_workspace_bytes(32) bytes of device memory, 16-byte aligned, that no other launch
 *   in flight uses (contents: don't care, before and after); C = 16: workspace may be NULL.
 *   packed: fv_pack_mrf_stage_split_f16 of the 18 Conv1d weights and biases -- w1[3 j + p], w2[3 j + p]: [C, C, k_j];
 *   b1 / b2: arrays of 9 pointers to [C] (entries, or the arrays, may be NULL); fv_packed_mrf_stage_floats floats
 *   (0 = shape not built).  Per pair: [conv1 image | conv2 image | b1 | b2 | 1 / row prescale of conv1 | of conv2].
 *   fold_w [C, 7] != NULL (HiFi-GAN's conv_post, hifigan.py:104-106, inside the launch; needs y = y_act = NULL):
 *       fold_y[B, 1, T] = post( conv1d( lrelu(((r_0 + r_1) + r_2) / out_div, act_slope); fold_w, zero padding 3 ) + fold_b )
 *   -- the same arithmetic, bit for bit, as fv_conv1d_fused on a stored y.
 */
int64_t fv_packed_mrf_stage_floats(int C, const int* k);
int fv_pack_mrf_stage_split_f16(const float* const* w1, const float* const* w2, const float* const* b1,
                                const float* const* b2, float* packed, int C, const int* k, int* range_flag, void* stream);
int64_t fv_mrf_stage_workspace_bytes(int C);
int fv_mrf_stage_split_f16(const float* x, const float* packed, float* y, float* y_act, int B, int C, int T, const int* k,
                           const int* dil, float slope, float out_div, int post, float act_slope, const float* fold_w,
                           const float* fold_b, float* fold_y, void* workspace, int64_t workspace_bytes, int* guard,
                           void* stream);
/*
 * The 32-channel stage as ONE launch of two block classes (csrc/mrfw_kernels.hpp, SPLIT): the three ResBlocks are
 * independent until the sum, so class A blocks run the 11-tap ResBlock alone and class B blocks the 3- and 7-tap ones, each
 * class on windows that overlap by its OWN reach (60 / 36 columns instead of 60 for all) and cost about half a window:
 *     y_s = r_0 + r_1,   y_r2 = r_2        (un-divided; the consumer forms ((r_0 + r_1) + r_2) / 3, e.g. the merged
 *                                           input of fv_plan_set_input_merge(add1 = y_r2, add2 = none, div = 3))
 * -- bit-identical to the pair launches' r_0, r_1, r_2 summed in that order.  C = 32, k = {3, 7, 11} in this order,
 * dil = {1, 3, 5}; anything else: FV_ERR_UNSUPPORTED.  x, y_s, y_r2 [B, 32, T], no aliasing; packed, workspace, guard: as
 * fv_mrf_stage_split_f16.  The launcher gives class A n_A and class B n_B of its blocks (n_A + n_B <= one per CU, at most
 * one per 128 columns, at most 256) so that the slower class's whole windows x window cost is smallest; a block's columns
 * lie inside one utterance, so fewer than 2 B blocks is FV_ERR_UNSUPPORTED (one block: use fv_mrf_stage_split_f16).
 */
int fv_mrf_stage_classes_f16(const float* x, const float* packed, float* y_s, float* y_r2, int B, int C, int T, const int* k,
                             const int* dil, float slope, void* workspace, int64_t workspace_bytes, int* guard, void* stream);

/*
 * Conv1d of the wide ResBlock stages with split-f16 operands (arithmetic: FV_PAIR_SPLIT_F16 above), n = 1..3
 * independent members in one launch -- the convs at the same position of the three ResBlocks of an MRF stage:
 *
 *     y_j = post( ( conv1d( lrelu(x_j, pre_slope); w_j, k_j taps, dilation dil, 'same' padding ) + bias_j
 *                   + res_j + add1_j + add2_j ) / out_div ),      y_act_j = lrelu(y_j, act_slope)
 *
 * pad_mode: FV_PAD_ZERO (the HiFi-GAN ResBlock convs) or FV_PAD_REFLECT (the dilated convs of MelGAN's
 * ResidualStack, modules.py:351-359: ReflectionPad1d((k-1)/2*dil) in front of a 3-tap conv; needs (k-1)/2*dil < T).
 * (modules.py:223-230: conv1 of a pair is res = add = NULL; conv2 is res = the pair's input; the last conv of a
 * stage's first block carries the MRF merge, hifigan.py:99-103, with add1 / add2 = the other blocks' results.)
 * C = Cin = Cout = 64, 128, 256 or 512, k_j in {3, 7, 11}, dil in {1, 3, 5} (and 9 with k_j = 3); x_j is read RAW (the activation is applied on
 * chip while the operand is split); packed_j: fv_pack_pair_weight_ex(C, k_j, FV_PAIR_SPLIT_F16) -- the packed
 * weights stream L2 -> LDS through a 4-stage ring (csrc/convh_kernels.hpp).  out_div / post apply to members with
 * add1 only.  Any T.
 */
int fv_conv1d_split_f16(int n, const float* const* x, const float* const* packed, const float* const* bias,
                        const float* const* res, const float* const* add1, const float* const* add2, float* const* y,
                        float* const* y_act, const int* k, int B, int C, int T, int dil, int pad_mode, float pre_slope,
                        float out_div, int post, float act_slope, int* guard, void* stream);

/*
 * ConvTranspose1d with split-f16 operands (arithmetic: FV_PAIR_SPLIT_F16 above) for the upsamplers whose kernel is two
 * strides long -- every one the reference builds (hifigan.py:45-46, melgan.py:37-39: kernel 2 s, padding s/2 + s%2,
 * output_padding s%2):
 *
 *     y = conv_transpose1d( lrelu(x, pre_slope); w [Cin, Cout, k], stride, pad, out_pad ) + bias,  y_act = lrelu(y, act_slope)
 *
 * (without y_act and act_slope != 1, y itself is stored activated).  Cin = 64, 128, 256 or 512; k = 2 stride, stride 2..16;
 * Cout * stride >= 64 (rows are padded to a multiple of 64, 64 input channels to 128); 0 <= pad <= stride; out_pad in [-stride, stride) (negative: CausalConvTranspose1d's
 * trim, modules.py:297-317).  Tout = (Tin-1)*stride - 2*pad + k + out_pad.  With n + pad = stride u + phase every
 * output sample has the two taps x[u], x[u-1]: one GEMM with rows (output channel, phase), weights streamed as in
 * fv_conv1d_split_f16 (csrc/convh_kernels.hpp, convt_kernel).  packed: fv_pack_conv_transpose1d_split_f16
 * (fv_packed_conv_transpose1d_split_floats floats; 0 = shape not supported).
 */
int64_t fv_packed_conv_transpose1d_split_floats(int Cin, int Cout, int k, int stride);
int fv_pack_conv_transpose1d_split_f16(const float* w, float* packed, int Cin, int Cout, int k, int stride, int* range_flag,
                                       void* stream);
int fv_conv_transpose1d_split_f16(const float* x, const float* packed, const float* bias, float* y, float* y_act, int B,
                                  int Cin, int Cout, int Tin, int k, int stride, int pad, int out_pad, float pre_slope,
                                  float act_slope, int* guard, void* stream);

/*
 * End of an MRF stage (hifigan.py:97-103): the LAST pairs of the three ResBlocks and the mean, one launch:
 *
 *     y = post( ( sum_{j<3} pair_j(x_j) ) / out_div ),   y_act = lrelu(y, act_slope)   (as fv_conv1d_fused)
 *
 * pair_j as in fv_resblock1_fused (taps 11 / 7 / 3 in any order).  The three results are summed inside
 * the fp32 accumulator rather than as ((r0 + r1) + r2): equal up to fp32 rounding of the additions.
 * Supported: C = 16 (the three weight sets stay resident in LDS); otherwise FV_ERR_UNSUPPORTED --
 * use fv_conv1d_fused for the first convs and the sum3 plan op / running-sum epilogues for the merge.
 */
int fv_mrf_stage(const float* const* x, const float* const* w1, const float* const* w2, const float* const* b1,
                 const float* const* b2, float* y, float* y_act, const int* k, int B, int C, int T, int dil,
                 float slope, float out_div, int post, float act_slope, void* stream);

/*
 * y = post( W1 * x + W2 * x2 + bias + res )    (two 1-tap convs that are summed, as ONE GEMM)
 *
 * Replaces ResidualStack's tail (modules.py:362-366,382): stack[4](act(h)) + skip_layer(c) --
 * the K range of the 1x1 conv is the concatenation of the two input tensors, so the skip
 * branch costs no launch, no [B,C,T] round trip through HBM and no separate add.
 *   x [B,Cin1,T], x2 [B,Cin2,T] (both already activated as the graph requires: there is no
 *   input activation here), packed = fv_pack_conv1d_weight of cat([W1, W2], dim=1)
 *   [Cout, Cin1+Cin2, 1], bias = b1 + b2 (or NULL), res [B,Cout,T] or NULL, Cout > 4.
 */
int fv_conv1d_2src_fused(const float* x, const float* x2, const float* packed, const float* bias,
                         const float* res, float* y, float* y_act, int B, int Cin1, int Cin2,
                         int Cout, int T, int post, float act_slope, void* stream);

/*
 * The same operator with split-f16 operands (arithmetic and domain: FV_PAIR_SPLIT_F16 above) for C -> C stacks,
 * C = 128, 256 or 512 -- MelGAN's and Basis-MelGAN's ResidualStack tails (modules.py:362-366,382):
 *
 *     y = post( W1 * lrelu(x, pre_slope) + W2 * x2 + bias + res ),   y_act = lrelu(y, act_slope)
 *
 * x is read RAW and activated on chip while it is split (nothing is hoisted into its producer), x2 is read as it is.
 * One GEMM over the K range [lrelu(x); x2] on the streamed-weight pipeline of fv_conv1d_split_f16 (csrc/convh_kernels.hpp
 * convg_kernel).  packed: fv_pack_conv1x1_2src_split_f16 of the two [C, C, 1] weights (fv_packed_conv1x1_2src_split_floats
 * floats; 0 = C not supported); bias = b1 + b2 or NULL.
 */
int64_t fv_packed_conv1x1_2src_split_floats(int C);
int fv_pack_conv1x1_2src_split_f16(const float* w1, const float* w2, float* packed, int C, int* range_flag, void* stream);
int fv_conv1x1_2src_split_f16(const float* x, const float* x2, const float* packed, const float* bias, const float* res,
                              float* y, float* y_act, int B, int C, int T, float pre_slope, int post, float act_slope,
                              int* guard, void* stream);

/*
 * MelGAN's ResidualStack (modules.py:351-382) as ONE launch, C = 32, 64, 128 or 256 channels, 3 taps, dilation 1, 3 or 9,
 * split-f16 operands (arithmetic and domain: FV_PAIR_SPLIT_F16 above):
 *
 *     y = post( W2 * lrelu( conv1d( pad( lrelu(x, slope) ); w_dilated, dil ) + bias_dilated, slope ) + Ws * x + bias_out )
 *
 * stack = [act, pad, Conv1d(C, C, 3, dilation), act, Conv1d(C, C, 1)] (modules.py:362-366), skip_layer = Conv1d(C, C, 1)
 * of the raw input (:377, :382); bias_out = stack[4].bias + skip_layer.bias or NULL; pad_mode FV_PAD_ZERO or
 * FV_PAD_REFLECT (`dil` samples on either side: the 'same' padding of the dilated conv).  The hidden tensor never
 * leaves the CU (csrc/convk_kernels.hpp); at 128 and 256 channels the result is bit-identical to fv_conv1d_split_f16 followed
 * by fv_conv1x1_2src_split_f16.  y_act (or NULL): lrelu(y, act_slope); without y_act and act_slope != 1, y itself is
 * stored activated.  packed: fv_pack_residual_stack_split_f16 of the three weights [C, C, 3], [C, C, 1], [C, C, 1]
 * (fv_packed_residual_stack_floats floats; 0 = shape not built).
 */
int64_t fv_packed_residual_stack_floats(int C, int k);
int fv_pack_residual_stack_split_f16(const float* w_dilated, const float* w_pointwise, const float* w_skip, float* packed,
                                     int C, int k, int* range_flag, void* stream);
int fv_residual_stack_split_f16(const float* x, const float* packed, const float* bias_dilated, const float* bias_out, float* y,
                                float* y_act, int B, int C, int T, int k, int dil, float slope, int pad_mode, int post,
                                float act_slope, int* guard, void* stream);

/*
 * y = post( conv_transpose1d(lrelu(x, pre_slope); w, stride, pad, out_pad) + bias )
 *
 * Replaces F.leaky_relu + torch.nn.ConvTranspose1d at hifigan.py:95-96,
 * multiband_hifigan.py:104-105, melgan.py:75-85, basis_melgan.py:86-97, and --
 * with Cout = 1, k = L, stride = L/2, pad = 0, packed from W^T -- the
 * F.linear + overlap_and_add pair of BasisSignalLayer (modules.py:264-267,
 * :34-73).  x [B,Cin,Tin] -> y [B,Cout,Tout],
 * Tout = (Tin-1)*stride - 2*pad + k + out_pad; -stride <= out_pad < stride: a negative out_pad drops
 * the tail of the output -- CausalConvTranspose1d (modules.py:297-317) is pad = 0, out_pad = -stride.
 */
int fv_conv_transpose1d_fused(const float* x, const float* packed, const float* bias,
                              float* y, float* y_act, int B, int Cin, int Cout, int Tin,
                              int k, int stride, int pad, int out_pad, float pre_slope,
                              int post, float act_slope, void* stream);

/*
 * BasisSignalLayer + overlap_and_add (reference model/generator/modules.py:255-267, :34-73; Basis-MelGAN's last step,
 * basis_melgan.py:140-162): frames = weight W^T (F.linear, no bias), out[hop f + j] += frames[f, j], hop = L / 2.
 *   weight [B, C, F]: the trunk's output as it lies in memory (channel-major: the reference's transpose(1, 2) view);
 *   W [L, C]: basis_signal.layer.weight;   out [B, 1, hop (F - 1) + L]   (L = 30, C = 256: [B, 15 F + 15]).
 * One launch: the op is a ConvTranspose1d(C -> 1, kernel L, stride hop, pad 0) with weight W^T on the fp32-MFMA kernel
 * (fv_conv_transpose1d_fused); the [B, F, L] frame tensor is never materialised.  packed_basis: fv_pack_basis of W
 * (fv_packed_basis_floats(L, C) floats: the packed image and, behind it, the transposed weight it was made from).
 */
int64_t fv_packed_basis_floats(int L, int C);
int fv_pack_basis(const float* W, float* packed, int L, int C, void* stream);
int fv_basis_ola(const float* weight, const float* packed_basis, float* out, int B, int C, int F, int L, void* stream);

/*
 * y = post( conv1d( nearest_repeat(lrelu(x, pre_slope), rate); w, padding = pad ) + bias )
 *
 * Replaces the reference's UpsampleLayer (modules.py:160-177: Stretch2d nearest x rate,
 * then Conv1d(k, padding)), selected by `transposedconv: False`.  The repeat is never
 * materialised: taps that read the same input sample are summed at pack time
 * (fv_pack_upsample_conv1d_weight) and the layer runs as a short dense conv over
 * Cout*rate phase rows.  x [B,Cin,Tin] -> y [B,Cout,Tout], Tout = rate*Tin + 2*pad - (k-1).
 */
int64_t fv_packed_upsample_conv1d_floats(int Cout, int Cin, int k, int rate, int pad);
int fv_pack_upsample_conv1d_weight(const float* w, float* packed, int Cout, int Cin, int k,
                                   int rate, int pad, void* stream);
int fv_upsample_conv1d_fused(const float* x, const float* packed, const float* bias, float* y,
                             float* y_act, int B, int Cin, int Cout, int Tin, int k, int rate,
                             int pad, float pre_slope, int post, float act_slope, void* stream);

/*
 * PQMF.synthesis (model/generator/pqmf.py:121-135) in polyphase form.
 *   x [B,S,Tsub] sub-bands, h [S,ntaps] (= synthesis_filter[0]), y [B,S*Tsub].
 */
int fv_pqmf_synthesis(const float* x, const float* h, float* y, int B, int S, int ntaps,
                      int Tsub, void* stream);

/*
 * Multiband-HiFi-GAN's inference tail in ONE launch (multiband_hifigan.py:113-115,136 with pqmf.py:121-135):
 *
 *     y = pqmf_synthesis( post( conv1d( lrelu(x, pre_slope); w [S, Cin, k], zero padding pad ) + bias ) )
 *
 * conv_post's S = 4 activated sub-bands stay in LDS and feed the polyphase synthesis (ntaps = 63) directly: the
 * [B, S, T] sub-band tensor never exists and one launch disappears.  Same FMA order as fv_conv1d_fused followed by
 * fv_pqmf_synthesis: identical bits.  x [B, Cin, T]; packed: fv_pack_conv1d_weight of w; h [S, ntaps]; y [B, S * T].
 */
int fv_conv_post_pqmf(const float* x, const float* packed, const float* bias, const float* h, float* y, int B, int Cin,
                      int S, int T, int k, int pad, float pre_slope, int post, int ntaps, void* stream);

/*
 * PQMF.analysis (pqmf.py:108-119): ntaps-tap FIR per band over the zero-padded signal,
 * decimated by S; only the kept samples are computed.
 *   x [B,T] full band, h [S,ntaps] (= analysis_filter[:,0]), y [B,S,(T-S)/S+1].
 * Not on the inference path (the reference uses it for the multiband training loss); it is
 * here so the PQMF class is whole and for the analysis->synthesis reconstruction check.
 */
int fv_pqmf_analysis(const float* x, const float* h, float* y, int B, int S, int ntaps,
                     int64_t T, void* stream);

/*
 * The wav sink's arithmetic (data/audio.py:12-14 encode_16bits) on the device, per waveform
 * (row) of x [B,n]:  s = 32767 / max(0.01, max|x|) * rescale_out;  out = int16(trunc(x * s)).
 * peak [B] receives max|x| per row (device scratch, also an output).  scale_in_place != 0
 * also writes x * s back to x, the reference's in-place mutation of its argument.
 * Results equal numpy's for a float32 array bit for bit (tests/test_gpu_parity.py).
 */
int fv_encode_16bits(float* x, int16_t* out, float* peak, int B, int64_t n, float rescale_out,
                     int scale_in_place, void* stream);

/*
 * The reference's mel-spectrogram front end (data/audio.py:58-61 melspectrogram, hparams.py:4-15) in ONE launch,
 * per waveform (row) of x [B, n]:
 *   1. preemphasis p[0] = x[0], p[i] = x[i] - 0.97 x[i-1]                 (scipy lfilter, zero initial state)
 *   2. |STFT|: center=True with numpy 'reflect' padding by n_fft/2, periodic Hann of win_length centred in
 *      n_fft, hop; T = 1 + n / hop frames, bins 0..n_fft/2                  (librosa < 0.10 stft)
 *   3. mel = filters @ |STFT|, the Slaney-normalised mel filters of librosa.filters.mel(sr, n_fft, n_mels, fmin)
 *   4. out = clip((20 log10(max(1e-5, mel)) - ref_level_db(20) - min_level_db(-100)) / 100, 0, 1)
 * x: fp32 device [B, n]; mel: fp32 device [B, n_mels, T] (the generators' forward layout).
 * tables: fp32 device, FV_MEL_TABLE_FLOATS floats in the layout below, built in float64 on the host and rounded
 * once (fastvocoder_amd/audio.py mel_tables):
 *   [FV_MEL_TAB_WINDOW]   win_length window taps (the non-zero part of the padded window)
 *   [FV_MEL_TAB_TWIDDLE]  n_fft/2 complex (re, im) exp(-2 pi i t / (n_fft/2)), the packed complex FFT's twiddles
 *   [FV_MEL_TAB_SPLIT]    n_fft/2 complex exp(-2 pi i k / n_fft), the real-FFT split step's twiddles
 *   [FV_MEL_TAB_FILTERS]  n_mels x (first bin, bin count, offset into the weights), integers held as floats
 *   [FV_MEL_TAB_WEIGHTS]  each filter's non-zero weights, consecutive, at most FV_MEL_MAX_WEIGHTS in all
 * The kernel is specialised to the reference's parameters: sample_rate 24000, n_fft 2048, hop 240, win_length 1200,
 * n_mels 80, fmin 40; anything else returns FV_ERR_UNSUPPORTED.  n < n_fft/2 + 1 (too short to reflect-pad) or
 * B outside 1..65535 returns FV_ERR_INVALID_ARG.
 */
#define FV_MEL_TAB_WINDOW 0
#define FV_MEL_TAB_TWIDDLE 1200
#define FV_MEL_TAB_SPLIT 3248
#define FV_MEL_TAB_FILTERS 5296
#define FV_MEL_TAB_WEIGHTS 5536
#define FV_MEL_MAX_WEIGHTS 2050
#define FV_MEL_TABLE_FLOATS (FV_MEL_TAB_WEIGHTS + FV_MEL_MAX_WEIGHTS)
int fv_mel_table_floats(void);
int fv_melspectrogram(const float* x, float* mel, const float* tables, int B, int64_t n, int sample_rate, int n_fft,
                      int hop, int win_length, int n_mels, float fmin, void* stream);

/*
 * (added within v18: an additive entry, the version stays)
 * Sample-rate conversion by a rational ratio: the resampling inside the reference's load_wav (data/audio.py:17-18,
 * librosa.load(sr=...), with librosa < 0.10 resampy's kaiser_best: band-limited interpolation with a Kaiser-windowed
 * sinc) as a polyphase FIR, per row of x [B, n_in].  With g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g:
 *   n_out = ceil(n_in L / M)                                    (fv_resample_out_len; librosa.resample(fix=True))
 *   c, p = divmod(j M, L);   y[b, j] = sum_{t < 2 half + 2} table[t L + (j mod L)] * x[b, c - half + t]
 * with x = 0 outside [0, n_in).  The filter is the caller's: `table` holds, TAP-MAJOR, row r = j mod L of the
 * 2 half + 2 coefficients  scale h(scale (half - t + p_r / L)),  p_r = (r M) mod L  (fastvocoder_amd/audio.py
 * resample_tables builds it in float64 and rounds once; scale, half and h are its business, the kernel applies them).
 * x: device [B, n_in], fp32 (FV_PCM_F32) or 16-bit PCM (FV_PCM_S16, converted on load as s / 32768, which is exact:
 * a 16-bit file crosses PCIe at 2 bytes per sample); y: fp32 device [B, n_out]; table: fp32 device.
 * One launch; an output is one thread's fp32 FMA chain over its taps in increasing t, so its bits depend only on the
 * 2 half + 2 inputs around it and on j mod L -- not on the row, the batch size or the grid.  j M and c are 64-bit.
 * Limits: 1 <= L, M <= FV_RESAMPLE_MAX_FACTOR, 1 <= n_in <= FV_RESAMPLE_MAX_SAMPLES, B in 1..65535 (FV_ERR_INVALID_ARG,
 * as a wrong n_out); a table above FV_RESAMPLE_MAX_TABLE_FLOATS floats or a block's input window
 * floor((L - 1 + 255 M) / L) + 2 half + 2 above FV_RESAMPLE_MAX_WINDOW floats of LDS returns FV_ERR_UNSUPPORTED.
 */
#define FV_PCM_F32 0
#define FV_PCM_S16 1
#define FV_RESAMPLE_MAX_FACTOR (1 << 20)
#define FV_RESAMPLE_MAX_SAMPLES ((int64_t)1 << 40)
#define FV_RESAMPLE_MAX_TABLE_FLOATS (1 << 20)
#define FV_RESAMPLE_MAX_WINDOW 16384
int64_t fv_resample_out_len(int64_t n_in, int L, int M);
int fv_resample(const void* x, int x_format, float* y, const float* table, int B, int64_t n_in, int64_t n_out, int L,
                int M, int half, void* stream);

/*
 * Griffin-Lim: the reference's inv_mel_spectrogram (data/audio.py:66-95,179-190 with hparams.py as shipped, librosa < 0.10
 * semantics), the inverse direction of fv_melspectrogram.  Geometry n_fft 2048 / hop 240 / win_length 1200 (a periodic
 * Hann window centred in the frame) only; anything else returns FV_ERR_UNSUPPORTED.  Spectra and magnitudes are
 * FRAMES-MAJOR here, [B, T, 1025] (a frame's bins consecutive: a wave owns a frame), the transpose of librosa's
 * [1025, T]; complex values are (re, im) float pairs.
 *
 * tables: fp32 device, FV_GL_TABLE_FLOATS floats, 16-byte aligned, built in float64 on the host and rounded once
 * (fastvocoder_amd/audio.py griffin_lim_tables); the first three parts are fv_melspectrogram's:
 *   [FV_GL_TAB_WINDOW]   1200 window taps        [FV_GL_TAB_TWIDDLE]  1024 complex exp(-2 pi i t / 1024)
 *   [FV_GL_TAB_SPLIT]    1024 complex exp(-2 pi i k / 2048)           [FV_GL_TAB_WIN2]  the 1200 squared window taps
 *
 * fv_stft: y [B, n] -> spec [B, T, 1025] complex, T = 1 + n / 240: librosa.stft(y, 2048, 240, 1200), centred, numpy
 *   'reflect' padding by 1024 (n >= 1025).  One launch.
 * fv_istft: spec [B, T, 1025] complex -> y [B, 240 (T - 1)]: librosa.istft(D, hop_length=240, win_length=1200): inverse
 *   real FFT of each frame (Im of bins 0 and 1024 ignored), times the window, overlap-added, divided by the overlap-added
 *   squared window where that exceeds FLT_MIN, 1024 samples trimmed from each end.  T >= 2.  Two launches: the frames
 *   into the workspace ([B, T, 1200] floats, fv_istft_workspace_bytes), then a gather that sums each sample's (at most
 *   five) frames in increasing frame order -- no atomics: identical calls give identical bits.
 * fv_griffin_lim: S [B, T, 1025] magnitudes, phase0 [B, T, 1025] complex initial phases (exp(2 pi i u), u the
 *   reference's uniform draw), y [B, 240 (T - 1)]:  y = istft(S * phase0), then `iters` times
 *   y = istft(S * exp(i angle(stft(y)))), angle(0) = 0.  phase0 = NULL: the iterations start from the caller's y.
 *   T >= 6 (the iterate is reflect-padded).  Two launches per iteration (the projection with the frame resident in LDS,
 *   the overlap-add gather), all enqueued on `stream` without a host synchronisation; same workspace as fv_istft.
 *   Rows are independent: row b of a batched call has the bits of its single call.
 * fv_mel_to_linear: mel [B, 80, T] normalised mel (values clipped to [0, 1]), inv_basis [80, 1025] = pinv(mel filters)^T
 *   in fp32 -> S [B, T, 1025] = max(1e-10, pinv @ 10^((mel 100 - 100 + 20) / 20))^power (the dot products in float64).
 * fv_inv_preemphasis: out[b, i] = y[b, i] + coef out[b, i-1] (scipy lfilter([1], [1, -coef]), zero initial state) over
 *   rows of n samples, |coef| < 1, as a blocked scan whose carries are exact; out may be y.
 * y, workspace and tables must be 16-byte aligned, spec / phase0 8-byte aligned.
 */
#define FV_GL_TAB_WINDOW 0
#define FV_GL_TAB_TWIDDLE 1200
#define FV_GL_TAB_SPLIT 3248
#define FV_GL_TAB_WIN2 5296
#define FV_GL_TABLE_FLOATS (FV_GL_TAB_WIN2 + 1200)
#define FV_GL_MAX_FRAMES (1 << 20)
int fv_gl_table_floats(void);
int64_t fv_istft_workspace_bytes(int B, int T);
int64_t fv_griffin_lim_workspace_bytes(int B, int T);
int fv_stft(const float* y, float* spec, const float* tables, int B, int64_t n, int n_fft, int hop, int win_length,
            void* stream);
int fv_istft(const float* spec, float* y, const float* tables, int B, int T, int n_fft, int hop, int win_length,
             void* workspace, size_t workspace_bytes, void* stream);
int fv_griffin_lim(const float* S, const float* phase0, float* y, const float* tables, int B, int T, int iters,
                   int n_fft, int hop, int win_length, void* workspace, size_t workspace_bytes, void* stream);
int fv_mel_to_linear(const float* mel, const float* inv_basis, float* S, int B, int T, int n_mels, int n_freq,
                     float power, void* stream);
int fv_inv_preemphasis(const float* y, float* out, int B, int64_t n, float coef, void* stream);

/*
 * The reference's STFT magnitude (model/loss/stft_loss.py:16-39 stft: torch.stft with its defaults, then
 * sqrt(clamp(re^2 + im^2, min=1e-7))), per row of x [B, n]:
 *   center=True with numpy 'reflect' padding by n_fft/2 on each side (no edge repeat); the win_length window centred
 *   in n_fft (left offset (n_fft - win_length) / 2, zeros around it); T = 1 + n / hop frames; bins 0..n_fft/2;
 *   mag[b, t, k] = sqrt(max(re^2 + im^2, 1e-7)).
 * x: fp32 device [B, n]; mag: fp32 device [B, T, n_fft/2 + 1] (the reference's (B, #frames, #bins)).
 * table: fp32 device, fv_stft_table_floats(n_fft, win_length) floats, built in float64 on the host and rounded once
 * (fastvocoder_amd/loss/stft_loss.py stft_tables):
 *   [FV_STFT_TAB_TWIDDLE(n_fft)]  n_fft/2 complex (re, im) exp(-2 pi i t / (n_fft/2)), the packed complex FFT's twiddles
 *   [FV_STFT_TAB_SPLIT(n_fft)]    n_fft/2 complex exp(-2 pi i k / n_fft), the real-FFT split step's twiddles
 *   [FV_STFT_TAB_WINDOW(n_fft)]   the win_length window taps (torch.hann_window(win_length) by default)
 * n_fft must be 512, 1024 or 2048, hop >= 1 and 1 <= win_length <= n_fft, otherwise FV_ERR_UNSUPPORTED (and
 * fv_stft_table_floats returns FV_ERR_UNSUPPORTED).  n < n_fft/2 + 1 (too short to reflect-pad), a null pointer or
 * B outside 1..65535 returns FV_ERR_INVALID_ARG.  One launch.
 */
#define FV_STFT_MAX_RES 8
#define FV_STFT_TAB_TWIDDLE(n_fft) 0
#define FV_STFT_TAB_SPLIT(n_fft) (n_fft)
#define FV_STFT_TAB_WINDOW(n_fft) (2 * (n_fft))
int fv_stft_table_floats(int n_fft, int win_length);
int fv_stft_magnitude(const float* x, float* mag, const float* table, int B, int64_t n, int n_fft, int hop,
                      int win_length, void* stream);

/*
 * The per-utterance partial sums of the reference's multi-resolution STFT loss (model/loss/stft_loss.py:42-80
 * SpectralConvergenceLoss / LogSTFTMagnitudeLoss, :124-155 MultiResolutionSTFTLoss) for an estimate x and a target
 * y, both fp32 device [B, n].  With X, Y the fv_stft_magnitude magnitudes of x and y at resolution r
 * (n_fft[r], hop[r], win_length[r], tables[r]), summed over all T_r frames and n_fft[r]/2 + 1 bins:
 *   out[r, b, 0] = S_diff = sum (|Y| - |X|)^2
 *   out[r, b, 1] = S_ref  = sum |Y|^2
 *   out[r, b, 2] = S_log  = sum |ln|Y| - ln|X||
 * out: float64 device [R, B, 3].  The reference's batch-level terms are
 *   SC_r = sqrt(sum_b S_diff) / sqrt(sum_b S_ref),  mag_r = sum_b S_log / (B T_r (n_fft[r]/2 + 1)),
 * each averaged over the R resolutions (fastvocoder_amd/loss/stft_loss.py).  tables: a HOST array of R device
 * pointers, each table laid out as for fv_stft_magnitude; n_fft, hop, win_length: HOST arrays of R ints.
 * Two launches on `stream`: all resolutions' frames in one (the magnitudes never leave the chip; each block writes
 * three float64 partials to `workspace`), then a fixed-order float64 sum per (r, b).  No atomics: identical calls
 * return identical bits.  workspace: device memory of at least fv_stft_distance_workspace_bytes(B, n, R, n_fft, hop)
 * bytes (8-byte aligned).  Per-resolution parameters are checked as for fv_stft_magnitude (FV_ERR_UNSUPPORTED,
 * FV_ERR_INVALID_ARG for a short n); R outside 1..FV_STFT_MAX_RES, a small workspace, a null pointer or B outside
 * 1..65535 returns FV_ERR_INVALID_ARG.  fv_stft_distance_workspace_bytes returns a negative FV_ERR_* code for
 * arguments fv_stft_distance would refuse.
 */
int64_t fv_stft_distance_workspace_bytes(int B, int64_t n, int R, const int* n_fft, const int* hop);
int fv_stft_distance(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                     const int* n_fft, const int* hop, const int* win_length, double* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/*
 * The gradient of fv_stft_distance's sums with respect to the estimate x.  For a scalar L that depends on x through
 * out[r, b, 0] = S_diff and out[r, b, 2] = S_log (S_ref depends on y alone), with the caller's coefficients
 *   coef[r, b, 0] = dL/dS_diff,  coef[r, b, 1] = dL/dS_log        (fp32 device [R, B, 2], finite)
 * it writes gx = dL/dx, fp32 device [B, n].  Per bin, with (re, im) the spectrum of x and X, Y the magnitudes,
 *   G = coef0 * -2 (Y - X) + coef1 * -sign(ln Y - ln X) / X        (sign(0) = 0)
 *   dL/d(re, im) = G (re, im) / X where re^2 + im^2 > 1e-7, else 0 (the clamp passes no gradient)
 * then the adjoint of the windowed one-sided real FFT (n_fft * irfft of the bins with the interior bins halved, times
 * the window), the overlap-add of the frames at `hop`, the reflect padding folded back onto the samples it was read
 * from, and the sum over the resolutions.  x == y gives exactly 0.  The target has no gradient here.
 * Two launches on `stream`: one wave per frame transforms frame t of x and y, forms the bins' gradient in registers,
 * runs the inverse transform and writes the frame's win_length taps to `workspace`; then a gather sums, in a fixed
 * order, the taps that land on each sample and writes gx once.  No atomics: identical calls return identical bits, and
 * a row's gradient does not depend on B or on the other rows.  workspace: device memory of at least
 * fv_stft_distance_grad_workspace_bytes(...) = 4 B sum_r T_r win_length[r] bytes (4-byte aligned).  Parameter
 * checks and error codes as fv_stft_distance.
 */
int64_t fv_stft_distance_grad_workspace_bytes(int B, int64_t n, int R, const int* n_fft, const int* hop,
                                              const int* win_length);
int fv_stft_distance_grad(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                          const int* n_fft, const int* hop, const int* win_length, const float* coef, float* gx,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * fv_stft_magnitude in the discriminator's layout (model/discriminator/mfd.py:19-41 stft, which does not transpose):
 * mag: fp32 device [B, n_fft/2 + 1, T], mag[b, k, t].  The same FFT code and arithmetic as fv_stft_magnitude -- the
 * result is the transpose of its output bit for bit.  Arguments, checks and error codes as fv_stft_magnitude.
 * One launch.
 */
int fv_stft_magnitude_bins(const float* x, float* mag, const float* table, int B, int64_t n, int n_fft, int hop,
                           int win_length, void* stream);

/*
 * The adjoint of fv_stft_magnitude_bins: from gmag = dL/dmag, fp32 device [B, n_fft/2 + 1, T] in that function's
 * layout (T = 1 + n / hop), and the signal x [B, n] it was computed from, gx = dL/dx, fp32 device [B, n], all of it
 * written.  Per bin, with (re, im) the spectrum of frame t of x (the forward's own FFT code, so the clamp decisions
 * are the forward's),
 *   dL/d(re, im) = gmag[b, k, t] (re, im) / sqrt(max(re^2 + im^2, 1e-7)) where re^2 + im^2 > 1e-7, else 0
 * then, as in fv_stft_distance_grad, the adjoint of the windowed one-sided real FFT (n_fft * irfft of the bins with
 * the interior bins halved, times the window), the overlap-add of the frames at `hop` and the reflect padding folded
 * back.  gmag == 0 gives exactly 0; so does x == 0 (every bin is clamped).  table: as for fv_stft_magnitude.
 * Two launches on `stream`: one wave per frame (a block of 8 waves owns 16 consecutive frames and stages their gmag
 * tile in LDS with 64-byte runs per bin) writes the frame's win_length taps to `workspace`; then the gather of
 * fv_stft_distance_grad sums, frames in increasing order, the taps that land on each sample.  No atomics: identical
 * calls return identical bits, and a row's result does not depend on B or on the other rows.  workspace: device
 * memory of at least fv_stft_magnitude_bins_grad_workspace_bytes(...) = 4 B T win_length bytes (4-byte aligned).
 * Parameter checks and error codes as fv_stft_magnitude_bins (FV_ERR_UNSUPPORTED, FV_ERR_INVALID_ARG), before any
 * launch; a small workspace, or gx overlapping x, gmag or the workspace, returns FV_ERR_INVALID_ARG.  The
 * workspace function returns a negative FV_ERR_* code for arguments fv_stft_magnitude_bins_grad would refuse.
 */
int64_t fv_stft_magnitude_bins_grad_workspace_bytes(int B, int64_t n, int n_fft, int hop, int win_length);
int fv_stft_magnitude_bins_grad(const float* x, const float* gmag, const float* table, int B, int64_t n, int n_fft,
                                int hop, int win_length, float* gx, void* workspace, size_t workspace_bytes,
                                void* stream);

/*
 * The discriminators' strided grouped conv (model/discriminator/msd.py:67-80, mfd.py:85-98: torch.nn.Conv1d with
 * groups = Cin / 4, zero padding, then LeakyReLU):
 *     y[b, c, t] = lrelu( bias[c] + sum_{ci<4, j<k} w[c, ci, j] * x[b, 4 (c / (Cout/G)) + ci, t*stride + j - pad], slope )
 * with G = Cin / 4 groups and x read as 0 outside [0, Tin).  x [B,Cin,Tin]; w [Cout, 4, k] (the folded weight, as
 * fv_fold_weight_norm writes it; no packing); bias [Cout] or NULL; y [B,Cout,Tout],
 * Tout = (Tin + 2 pad - k) / stride + 1.  slope = 1 gives the raw conv.  y must not alias x or w.
 * Exact fp32 on the VALU, each output summed in the fixed order ci = 0..3, j = 0..k-1, then + bias: a row's values do
 * not depend on B or on the other rows.  Supported: Cin % 4 == 0 (4 input channels per group), Cout % (Cin / 4) == 0,
 * stride >= 1 and kernels up to the shared-memory budget of a block (every k = 10 stride + 1 or 6 stride + 1 with
 * stride <= 5); anything else returns FV_ERR_UNSUPPORTED.  Tout < 1, pad < 0, a null pointer or B outside 1..65535
 * returns FV_ERR_INVALID_ARG.  One launch.
 */
int fv_grouped_conv1d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Tin,
                      int k, int stride, int pad, float slope, void* stream);

/*
 * torch.nn.AvgPool1d(k, stride, padding, count_include_pad=False, ceil_mode=False) on `rows` rows of x
 * (model/discriminator/msd.py:150, 207: the input of every MelGAN scale after the first):
 *     y[r, t] = (sum of x[r, i] for i in [t*stride - pad, t*stride - pad + k) and 0 <= i < Tin) / (number of such i)
 * x [rows, Tin]; y [rows, Tout], Tout = (Tin + 2 pad - k) / stride + 1; fp32 sum in order of i, one division.
 * k >= 1, stride >= 1, 0 <= pad <= k / 2 (torch's own limit) and Tout >= 1, else FV_ERR_INVALID_ARG (likewise for a
 * null pointer, aliasing or rows < 1).  One launch.
 */
int fv_avg_pool1d(const float* x, float* y, int rows, int64_t Tin, int k, int stride, int pad, void* stream);

/*
 * Per-utterance sums behind the discriminator scores of the reference's training loop (bin/train.py:97-117
 * adversarial and feature-map loss, :157-169 discriminator loss) for M pairs of feature maps (e_m the estimate's,
 * r_m the real signal's), each pair fp32 device [B, n_m] rows (a map [B, C, T] has n_m = C T); per map and row b:
 *   out[m, b, 0] = sum |e - r|
 *   out[m, b, 1] = sum (e - 1)^2
 *   out[m, b, 2] = sum e^2
 *   out[m, b, 3] = sum (r - 1)^2
 * out: float64 device [M, B, 4].  e, r: HOST arrays of M device pointers; n: HOST array of M element counts.
 * Two launches on `stream`: every map's elements in one (each block writes four float64 partials to `workspace`),
 * then a fixed-order float64 sum per (m, b).  No atomics: identical calls return identical bits.  workspace: device
 * memory of at least fv_disc_score_workspace_bytes(B, M, n) bytes (8-byte aligned).  M outside
 * 1..FV_DISC_MAX_MAPS, n_m < 1, a small workspace, a null pointer or B outside 1..65535 returns FV_ERR_INVALID_ARG;
 * fv_disc_score_workspace_bytes returns a negative FV_ERR_* code for arguments fv_disc_score_sums would refuse.
 */
#define FV_DISC_MAX_MAPS 48
int64_t fv_disc_score_workspace_bytes(int B, int M, const int64_t* n);
int fv_disc_score_sums(const float* const* e, const float* const* r, const int64_t* n, int M, int B, double* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * The input gradient of the multi-scale discriminator (model/discriminator/msd.py) under the adversarial and
 * feature-map terms of bin/train.py:97-117; additions of ABI 18, no existing entry changes.  Exact fp32, no atomics:
 * every element is summed by one thread in a fixed order, so identical calls return identical bits and a row's values
 * do not depend on B or on the grid.  All entries launch on `stream` and own no device memory.
 *
 * fv_disc_map_grad: the gradient in front of a layer's LeakyReLU from the gradient behind it,
 *     g_pre[i] = (g_up[i] + g_map[i]) * (y[i] > 0 ? 1 : slope),   i < n
 * g_up: what the layer above hands down; g_map: what the loss puts on this layer's own map; either may be NULL (not
 * both).  y: the layer's stored output (the sign survives a positive slope; y == 0 takes `slope`, as torch's
 * leaky_relu backward); NULL with slope = 1 gives the plain sum (the last layer has no activation).  One launch.
 *
 * fv_grouped_conv1d_input_grad: the data gradient of fv_grouped_conv1d with fv_disc_map_grad as its load stage,
 *     dx[b, 4 g + ci, i] = sum_{oc in group g} sum_{j : (i + pad - j) % stride == 0, 0 <= (i + pad - j) / stride < Tout}
 *                            w[oc, ci, j] * g_pre[b, oc, (i + pad - j) / stride]
 * g_up, g_map, y [B,Cout,Tout] as above (the masked gradient is never written to memory); w [Cout, 4, k], the
 * forward's tensor; dx [B,Cin,Tin], all of it written: positions past the last window ((Tin + 2 pad - k) / stride
 * floors) receive exactly 0.  Evaluated polyphase (an input position meets only the taps of its phase
 * (i + pad) % stride), each element summed oc ascending, then j ascending.  Supported shapes and error codes as
 * fv_grouped_conv1d (FV_ERR_UNSUPPORTED first, before any launch); slope != 1 without y, both gradients NULL or dx
 * aliasing an input return FV_ERR_INVALID_ARG.  One launch.
 *
 * fv_reflect_pad_fold: the adjoint of ReflectionPad1d(P) on rows of T samples, from gp [rows, T + 2 P]:
 *     dx[r, i] = gp[i + P] + (1 <= i <= P ? gp[P - i] : 0) + (T - 1 - P <= i <= T - 2 ? gp[P + 2 (T - 1) - i] : 0)
 * summed in that order.  T > P (torch's own limit for the pad), else FV_ERR_INVALID_ARG.  One launch.
 *
 * fv_avg_pool1d_input_grad: the adjoint of fv_avg_pool1d: g [rows, Tout] -> dx [rows, Tin],
 *     dx[r, i] = sum over t ascending with t*stride - pad <= i < t*stride - pad + k of g[r, t] / count(t)
 * (count(t): the window's samples inside [0, Tin)); a gather over at most ceil(k / stride) windows.  Arguments and
 * checks as fv_avg_pool1d.  One launch.
 *
 * fv_disc_score_grad: the gradient of the sums of fv_disc_score_sums with respect to the estimate's maps, every map
 * in one launch.  e, r, g: HOST arrays of M device pointers ([B, n_m] rows each; g[m] NULL skips the map); n: HOST
 * array of M element counts; coef: HOST array [M, 3] of (c_l1, c_adv, c_fake) per map:
 *     g_m[b, i] = c_l1 * sign(e - r) + 2 c_adv (e - 1) + 2 c_fake e,      sign(0) = 0
 * The coefficients carry the means, the reference's divisors and the incoming gradient of the terms.  Checks as
 * fv_disc_score_sums.
 */
int fv_disc_map_grad(const float* g_up, const float* g_map, const float* y, float* g_pre, int64_t n, float slope,
                     void* stream);
int fv_grouped_conv1d_input_grad(const float* g_up, const float* g_map, const float* y, const float* w, float* dx,
                                 int B, int Cin, int Cout, int Tin, int k, int stride, int pad, float slope,
                                 void* stream);
int fv_reflect_pad_fold(const float* gp, float* dx, int rows, int64_t T, int P, void* stream);
int fv_avg_pool1d_input_grad(const float* g, float* dx, int rows, int64_t Tin, int k, int stride, int pad,
                             void* stream);
int fv_disc_score_grad(const float* const* e, const float* const* r, float* const* g, const int64_t* n,
                       const float* coef, int M, int B, void* stream);

/*
 * The parameter gradient of the multi-scale discriminator (bin/train.py:143-188, the discriminator's update);
 * additions of ABI 18, no existing entry changes.  Exact fp32, no atomics: the reduction over (b, t) is cut into a
 * number of splits that depends on the shape alone, a first launch writes every split's partial sums to `workspace`,
 * a second adds them in ascending order, so identical calls return identical bits.  Workgroups never wait on each
 * other.  workspace: device memory of at least fv_conv_weight_grad_workspace_bytes(...) bytes (4-byte aligned), which
 * returns a negative FV_ERR_* code for arguments the entry itself would refuse; its contents on entry do not matter.
 *
 * fv_conv1d_weight_grad: the weight gradient of a dense stride-1 conv with zero or reflection padding,
 *     dw[co, ci, j] = sum_{b, t} g_pre[b, co, t] * xpad[b, ci, t + j],      db[co] = sum_{b, t} g_pre[b, co, t]
 * g_pre [B,Cout,Tout], Tout = Tin + 2 pad - k + 1, the gradient in front of the layer's LeakyReLU as fv_disc_map_grad
 * writes it; x [B,Cin,Tin] the layer's stored input, padded by indexing (pad_mode FV_PAD_ZERO or FV_PAD_REFLECT);
 * dw [Cout,Cin,k]; db [Cout] or NULL (dw may be NULL when db is not).  Cout >= 64 with Cin k >= 64 runs as a GEMM on
 * v_mfma_f32_32x32x2_f32 (each element one k-ordered fmaf chain per split), every other shape as a plain reduction.
 * Any Cin, Cout, k >= 1 with Cin Cout k < 2^31; another pad_mode returns FV_ERR_UNSUPPORTED.  Tout < 1, pad < 0, a
 * reflection pad >= Tin, a null pointer, a result aliasing an input, a small workspace or B outside 1..65535 returns
 * FV_ERR_INVALID_ARG.
 *
 * fv_grouped_conv1d_weight_grad: the weight gradient of fv_grouped_conv1d,
 *     dw[oc, ci, j] = sum_{b, t} g_pre[b, oc, t] * x[b, 4 g + ci, t stride + j - pad]      (oc in group g)
 * with x read as 0 outside [0, Tin); dw [Cout,4,k]; db as above.  Exact fp32 on the VALU.  Supported shapes and error
 * codes as fv_grouped_conv1d_input_grad (FV_ERR_UNSUPPORTED first, before any launch).
 *
 * fv_weight_norm_grad: the adjoint of fv_fold_weight_norm.  Per row r of dw, v [dim0, inner] and g [dim0]:
 *     dot = <dw_r, v_r>, n = |v_r|;   dg[r] = dot / n;   dv_r = (g[r] / n) (dw_r - (dot / n^2) v_r)
 * dv or dg may be NULL (not both).  One launch, one block per row, fixed order.
 */
int64_t fv_conv_weight_grad_workspace_bytes(int grouped, int B, int Cin, int Cout, int Tin, int k, int stride, int pad,
                                            int pad_mode);
int fv_conv1d_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout, int Tin,
                          int k, int pad, int pad_mode, void* workspace, size_t workspace_bytes, void* stream);
int fv_grouped_conv1d_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout,
                                  int Tin, int k, int stride, int pad, void* workspace, size_t workspace_bytes,
                                  void* stream);
int fv_weight_norm_grad(const float* dw, const float* v, const float* g, float* dv, float* dg, int dim0, int64_t inner,
                        void* stream);

/*
 * The multi-period discriminator's convs (model/discriminator/mpd.py:131-164 DiscriminatorP).  A map [B, C, H, p] is
 * contiguous (flattened time n = h p + c); additions of ABI 18, no existing entry changes.
 *
 * fv_mpd_conv_first: the first layer, Conv2d(1, 32, (5, 1), (3, 1), padding (2, 0)) + LeakyReLU, straight from the
 * waveform x [B, T]: the reflect tail pad to a multiple of `period` (n_pad = period - T % period samples, flat index
 * n >= T reads x[2 (T - 1) - n]) and the [H, period] view are address arithmetic, no padded copy exists.
 *     y[b, co, h', c] = lrelu( bias[co] + sum_{j<5} w[co, j] * xpad[b, (3 h' + j - 2) period + c], slope )
 * with zeros for rows outside [0, H), H = (T + n_pad) / period.  w [32, 5] (the folded weight); bias [32] or NULL;
 * y [B, 32, H', period], H' = (H - 1) / 3 + 1.  Exact fp32 on the VALU, summed j = 0..4, then + bias.
 *
 * fv_period_conv: Conv2d(Cin, Cout, (5, 1), (3, 1), padding (2, 0)) + LeakyReLU on a map x [B, Cin, H, period]:
 *     y[b, co, h', c] = lrelu( bias[co] + sum_{ci, j<5} w[co, ci, j] * x[b, ci, 3 h' + j - 2, c], slope )
 * y [B, Cout, H', period].  packed: fv_pack_period_conv of the folded weight [Cout, Cin, 5]
 * (fv_packed_period_conv_floats(Cout, Cin) floats; 0 for an unsupported shape).  An implicit GEMM on the exact-fp32
 * matrix instructions, summed in the fixed order (ci, ci + 1) pairs ascending, j = 0..4, then + bias: a row's values
 * do not depend on B, on the grid or on any switch.  y must not alias x.
 *
 * Supported: period 2, 3, 5, 7 or 11; Cin 32, 128 or 512; Cout 128, 512 or 1024; anything else returns
 * FV_ERR_UNSUPPORTED (checked before everything else: nothing is launched).  A null pointer, aliasing, B outside
 * 1..65535, T < 1, n_pad >= T (torch's reflect pad refuses it too), H < 1 or 2^31 flattened samples and more return
 * FV_ERR_INVALID_ARG.  One launch each.
 */
int fv_mpd_conv_first(const float* x, const float* w, const float* bias, float* y, int B, int64_t T, int period,
                      float slope, void* stream);
int64_t fv_packed_period_conv_floats(int Cout, int Cin);
int fv_pack_period_conv(const float* w, float* packed, int Cout, int Cin, void* stream);
int fv_period_conv(const float* x, const float* packed, const float* bias, float* y, int B, int Cin, int Cout, int H,
                   int period, float slope, void* stream);

/*
 * The input gradient of the multi-period discriminator (model/discriminator/mpd.py:131-164) under the adversarial and
 * feature-map terms of bin/train.py:97-117; additions of ABI 18, no existing entry changes.  Exact fp32, no atomics:
 * every element is summed by one lane in a fixed order, so identical calls return identical bits and a row's values do
 * not depend on B or on the grid.  Both entries launch on `stream` and own no device memory.  The two stride-1 layers
 * (1024 -> 1024 at dilation p, conv_post) need no entry of their own: their data gradients are fv_conv1d_fused on
 * flipped, transposed weights (dilation p, padding 2 p and p) behind fv_disc_map_grad.
 *
 * fv_period_conv_input_grad: the data gradient of fv_period_conv with fv_disc_map_grad as its load stage,
 *     dx[b, ci, r, c] = sum_co sum_{j : (r + 2 - j) % 3 == 0, 0 <= (r + 2 - j) / 3 < Hout}
 *                         w[co, ci, j] * g_pre[b, co, (r + 2 - j) / 3, c]
 * g_up, g_map, y [B, Cout, Hout, period], Hout = (H - 1) / 3 + 1, as fv_disc_map_grad takes them (either gradient
 * may be NULL, not both; y is the layer's stored output, NULL with slope = 1); the masked gradient
 * g_pre = (g_up + g_map) * (y > 0 ? 1 : slope) is never written to memory.  packed: fv_pack_period_conv_grad of the
 * folded weight [Cout, Cin, 5] (fv_packed_period_conv_grad_floats(Cout, Cin) floats; 0 for an unsupported shape).
 * dx [B, Cin, H, period], all of it written.  Evaluated polyphase as an implicit GEMM on the exact-fp32 matrix
 * instructions (M = Cin, N = flattened positions, K = Cout x the taps of a phase): with r + 2 = 3 m + ph an input row
 * meets tap ph at output row m and tap ph + 3 at row m - 1; each element is summed over the pairs (co, co + 1)
 * ascending, tap ph before tap ph + 3.  One launch.
 *
 * fv_mpd_first_input_grad: the gradient of fv_mpd_conv_first down to the waveform, the adjoint of the reflect tail
 * folded in.  g_up, g_map, y0 [B, 32, H1, period] as above; w [32, 5] (the folded weight); dx [B, T]:
 *     dx[b, i] = P(i) + (T - 1 - n_pad <= i <= T - 2 ? P(2 (T - 1) - i) : 0)
 * P(n): the gradient of the padded flat sample n = (r, c), summed co ascending, then the taps of n's phase ascending;
 * the sample's own position first, then its mirror.  One thread per sample, VALU.  One launch.
 *
 * Supported: period 2, 3, 5, 7 or 11; (Cin, Cout) = (32, 128), (128, 512) or (512, 1024); anything else returns
 * FV_ERR_UNSUPPORTED (checked before everything else: nothing is launched).  Both gradients NULL, another null
 * pointer, slope != 1 without y, dx aliasing an input, B outside 1..65535, H < 1, T < 1, n_pad >= T or 2^31
 * flattened samples and more return FV_ERR_INVALID_ARG.
 */
int64_t fv_packed_period_conv_grad_floats(int Cout, int Cin);
int fv_pack_period_conv_grad(const float* w, float* packed, int Cout, int Cin, void* stream);
int fv_period_conv_input_grad(const float* g_up, const float* g_map, const float* y, const float* packed, float* dx,
                              int B, int Cin, int Cout, int H, int period, float slope, void* stream);
int fv_mpd_first_input_grad(const float* g_up, const float* g_map, const float* y0, const float* w, float* dx, int B,
                            int64_t T, int period, float slope, void* stream);

/*
 * The parameter gradient of the multi-period discriminator (bin/train.py:143-188, the discriminator's update);
 * additions of ABI 18, no existing entry changes.  Exact fp32, no atomics, and the scheme of fv_conv1d_weight_grad: a
 * number of splits that depends on the shape alone, a first launch that writes every split's partial sums to
 * `workspace`, a second that adds them in ascending order, so identical calls return identical bits.  workspace: device
 * memory of at least fv_..._workspace_bytes(...) bytes (4-byte aligned), which returns a negative FV_ERR_* code for
 * arguments the entry itself would refuse; its contents on entry do not matter.
 *
 * fv_period_conv_weight_grad: the weight and bias gradient of a (k, 1) conv along H with zero padding (k - 1) / 2,
 *     dw[co, ci, j] = sum_{b, h', c} g_pre[b, co, h', c] * x[b, ci, stride h' + j - (k - 1) / 2, c]
 *     db[co]        = sum_{b, h', c} g_pre[b, co, h', c]
 * g_pre [B, Cout, H', period], H' = (H - 1) / stride + 1, the gradient in front of the layer's LeakyReLU as
 * fv_disc_map_grad writes it; x [B, Cin, H, period] the layer's stored input, rows outside [0, H) read as 0;
 * dw [Cout, Cin, k]; db [Cout] or NULL (dw may be NULL when db is not).  Cout >= 64 with Cin k >= 64 runs as a GEMM
 * [Cout] x [Cin k] over B H' period on v_mfma_f32_32x32x2_f32 in units of 32 flat positions h' period + c (each
 * element one position-ordered fmaf chain per split), every other shape (conv_post) as a plain reduction in units of
 * 1024 positions.  Supported: period 2, 3, 5, 7 or 11; k 1, 3 or 5; stride 1, 2 or 3; Cin Cout k < 2^31; anything else
 * returns FV_ERR_UNSUPPORTED before any launch.  A null pointer, a result aliasing an input, a small workspace, H < 1,
 * B outside 1..65535 or a map of 2^31 words and more returns FV_ERR_INVALID_ARG.
 *
 * fv_mpd_first_weight_grad: the gradient of fv_mpd_conv_first's weight [32, 5] and bias [32], straight from the
 * waveform x [B, T]: the reflect tail and the [H, period] view are address arithmetic.  g_pre [B, 32, H1, period].
 * A block reduction per output channel.  Checks as fv_mpd_first_input_grad.
 */
int64_t fv_period_conv_weight_grad_workspace_bytes(int B, int Cin, int Cout, int H, int period, int k, int stride);
int fv_period_conv_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout, int H,
                               int period, int k, int stride, void* workspace, size_t workspace_bytes, void* stream);
int64_t fv_mpd_first_weight_grad_workspace_bytes(int B, int64_t T, int period);
int fv_mpd_first_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int64_t T, int period,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * The parameter gradient of the HiFi-GAN generators (model/generator/hifigan.py:92-106 under bin/train.py:67-136, the
 * generator's update); additions of ABI 18, no existing entry changes.  Exact fp32 on v_mfma_f32_32x32x2_f32 (32
 * channels and more) / v_mfma_f32_16x16x4_f32 (fewer), no atomics, workgroups never wait on each other.  The two
 * weight gradients follow the scheme of fv_conv1d_weight_grad: a number of splits that depends on the shape alone, a
 * first launch that writes every split's partial sums to `workspace`, a second that adds them in ascending order, so
 * identical calls return identical bits.  workspace: device memory of at least fv_..._workspace_bytes(...) bytes
 * (4-byte aligned), which returns a negative FV_ERR_* code for arguments the entry itself would refuse; its contents
 * on entry do not matter.
 *
 * fv_conv1d_weight_grad_dilated: the weight and bias gradient of a dense stride-1 dilated conv with zero padding,
 *     dw[co, ci, j] = sum_{b, t} g_pre[b, co, t] * xa[b, ci, t + j dil - pad],      db[co] = sum_{b, t} g_pre[b, co, t]
 * g_pre [B,Cout,Tout], Tout = Tin + 2 pad - dil (k - 1); xa [B,Cin,Tin] the conv's input as it saw it (after the
 * activation in front of it), read as 0 outside [0, Tin); dw [Cout,Cin,k] or NULL; db [Cout] or NULL (not both).  The
 * GEMM [Cout] x [Cin k] over B Tout for every channel count; the dilated read is resolved while the operand is
 * staged.  Cin, Cout, k, dil >= 1 with Cin Cout k < 2^31, else FV_ERR_UNSUPPORTED.  Tout < 1, pad < 0, a null pointer,
 * a result aliasing an input, a small workspace, B outside 1..65535 or a map of 2^30 words and more returns
 * FV_ERR_INVALID_ARG.
 *
 * fv_conv_transpose1d_input_grad: the data gradient of ConvTranspose1d (w [Cin,Cout,k], the forward's folded weight as
 * it lies in memory; stride s, padding p, output padding op; Tout = (Tin - 1) s - 2 p + k + op),
 *     dxa[b, ci, i] = sum_co sum_j w[ci, co, j] * g[b, co, i s + j - p]          (g read as 0 outside [0, Tout))
 * g [B,Cout,Tout]; dxa [B,Cin,Tin], all of it written.  The GEMM [Cin] x [B Tin] over Cout k, each element one
 * (co, j)-ordered fmaf chain: a row's values do not depend on B or on the grid.  One launch.
 *
 * fv_conv_transpose1d_weight_grad: its weight and bias gradient,
 *     dw[ci, co, j] = sum_{b, i} xa[b, ci, i] * g[b, co, i s + j - p],           db[co] = sum_{b, n} g[b, co, n]
 * xa [B,Cin,Tin] the layer's input as it saw it; dw [Cin,Cout,k] or NULL; db [Cout] or NULL (not both).  The GEMM
 * [Cin] x [Cout k] over B Tin; the stride-s gather of g is resolved while the operand is staged.  Any k, s >= 1, p >= 0
 * and op with Tout >= 1 (k % s != 0 and k > 2 s included); error codes as fv_conv1d_weight_grad_dilated.
 *
 * The elementwise steps of the walk, one launch each, n elements:
 * fv_tanh_grad:            out = g (1 - y y)                                   (y = tanh(z): the gradient in front of it)
 * fv_residual_merge_grad:  out = [acc +] (g_y + (x > 0 ? 1 : slope) d)         (x_next = x + conv(lrelu(x, slope)): the
 *                          gradient of x from g_y = dL/dx_next and the conv's data gradient d; acc, or NULL: the sum of
 *                          the other ResBlocks' input gradients of the stage).  out may alias g_y, d or acc.
 * fv_grad_div:             out = g / div                                       (the MRF mean's adjoint; a true division)
 */
int64_t fv_conv1d_weight_grad_dilated_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad);
int fv_conv1d_weight_grad_dilated(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                  int Tin, int k, int dil, int pad, void* workspace, size_t workspace_bytes,
                                  void* stream);
int fv_conv_transpose1d_input_grad(const float* g, const float* w, float* dxa, int B, int Cin, int Cout, int Tin, int k,
                                   int stride, int pad, int out_pad, void* stream);
int64_t fv_conv_transpose1d_weight_grad_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int stride, int pad,
                                                        int out_pad);
int fv_conv_transpose1d_weight_grad(const float* g, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                    int Tin, int k, int stride, int pad, int out_pad, void* workspace,
                                    size_t workspace_bytes, void* stream);
int fv_tanh_grad(const float* g, const float* y, float* out, int64_t n, void* stream);
int fv_residual_merge_grad(const float* g_y, const float* d, const float* x, const float* acc, float* out, int64_t n,
                           float slope, void* stream);
int fv_grad_div(const float* g, float* out, int64_t n, float div, void* stream);

/*
 * The convs behind a ReflectionPad1d (MelGAN's ResidualStack, model/generator/modules.py:320-382, and its two k = 7 edge
 * convs, melgan.py:61-63 and modules.py:76-89); additions of ABI 18, no existing entry changes.  The padded tensor is
 * never built.  With r(i) = -i for i < 0, 2 (T - 1) - i for i >= T and i otherwise (T = Tin, pad < Tin):
 *
 * fv_conv1d_weight_grad_dilated_mode: fv_conv1d_weight_grad_dilated with a pad_mode, FV_PAD_ZERO (the same kernels, the
 * same bits as that entry) or FV_PAD_REFLECT:
 *     dw[co, ci, j] = sum_{b, t} g_pre[b, co, t] * xa[b, ci, r(t + j dil - pad)],   db[co] = sum_{b, t} g_pre[b, co, t]
 * The mirrored index is resolved while the operand is staged, where the dilated read is resolved.  Error codes as
 * fv_conv1d_weight_grad_dilated; another pad_mode, or FV_PAD_REFLECT with pad >= Tin, returns FV_ERR_INVALID_ARG.
 *
 * fv_conv1d_input_grad_reflect: the data gradient of y = conv(reflection_pad(xa, pad), W, dil) in one launch,
 *     dxa[b, ci, i] = sum_{p in [0, T + 2 pad), r(p - pad) = i} sum_{co, j} W[co, ci, j] * g[b, co, p - j dil]
 * (g [B,Cout,Tout], Tout = Tin + 2 pad - dil (k - 1), read as 0 outside [0, Tout)); wt [Cin,Cout,k] is the forward's
 * folded weight with its first two axes swapped; dxa [B,Cin,Tin], all of it written.  The GEMM [Cin] x [B Tin] over
 * Cout k whose operand of column i is the sum of its gathers in the fixed order straight (p = i + pad), left mirror
 * (p = pad - i, 1 <= i <= pad), right mirror (p = pad + 2 (T - 1) - i, T - 1 - pad <= i <= T - 2): each element one
 * (co, j)-ordered fmaf chain, a row's values do not depend on B or on the grid.  pad >= Tin, Tout < 1, a null pointer
 * or a result aliasing an input returns FV_ERR_INVALID_ARG.
 */
int64_t fv_conv1d_weight_grad_dilated_mode_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad,
                                                           int pad_mode);
int fv_conv1d_weight_grad_dilated_mode(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin,
                                       int Cout, int Tin, int k, int dil, int pad, int pad_mode, void* workspace,
                                       size_t workspace_bytes, void* stream);
int fv_conv1d_input_grad_reflect(const float* g, const float* wt, float* dxa, int B, int Cin, int Cout, int Tin, int k,
                                 int dil, int pad, void* stream);

/*
 * The generators' weight gradients with bf16 operands (the Python side's grad_precision = "bf16"); additions of ABI 18,
 * no existing entry changes.  With bf16(.) the round-to-nearest-even of an fp32 value to bfloat16:
 *
 * fv_conv1d_weight_grad_dilated_bf16: fv_conv1d_weight_grad_dilated_mode on rounded operands,
 *     dw[co, ci, j] = sum_{b, t} bf16(g_pre[b, co, t]) * bf16(xa[b, ci, r(t + j dil - pad)])     (fp32 accumulation)
 *     db[co]        = sum_{b, t} g_pre[b, co, t]                                                 (un-rounded)
 * fv_conv_transpose1d_weight_grad_bf16: fv_conv_transpose1d_weight_grad in the same way,
 *     dw[ci, co, j] = sum_{b, i} bf16(xa[b, ci, i]) * bf16(g[b, co, i s + j - p]),    db[co] = sum_{b, n} g[b, co, n]
 * The rounding is applied to the value the kernel stages: a padded zero stays zero, a reflected sample is the rounded
 * sample.  The products are exact in fp32 (v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16), so dw differs from the
 * fp32 sum of the rounded products by the order of the additions alone; bf16 has fp32's exponent range, there is no
 * scaling.  Shapes, index arithmetic, tensors, error codes and the split / record / combine scheme are those of the
 * fp32 entries (units of 64 reduction steps instead of 32, so the workspace size and db's last bits may differ from
 * theirs): S is a function of the shape alone, identical calls return identical bits, the workspace's contents do not
 * matter, no atomics, no waiting between workgroups.  Two launches.
 */
int64_t fv_conv1d_weight_grad_dilated_bf16_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad,
                                                           int pad_mode);
int fv_conv1d_weight_grad_dilated_bf16(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin,
                                       int Cout, int Tin, int k, int dil, int pad, int pad_mode, void* workspace,
                                       size_t workspace_bytes, void* stream);
int64_t fv_conv_transpose1d_weight_grad_bf16_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int stride,
                                                             int pad, int out_pad);
int fv_conv_transpose1d_weight_grad_bf16(const float* g, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                         int Tin, int k, int stride, int pad, int out_pad, void* workspace,
                                         size_t workspace_bytes, void* stream);

/*
 * The multi-period discriminator's weight gradients with bf16 operands (DiscriminatorP.grad_precision = "bf16");
 * additions of ABI 18, no existing entry changes.
 *
 * fv_period_conv_weight_grad_bf16: fv_period_conv_weight_grad on rounded operands, the same arguments,
 *     dw[co, ci, j] = sum_{b, h', c} bf16(g_pre[b, co, h', c]) * bf16(x[b, ci, stride h' + j - (k - 1) / 2, c])
 *     db[co]        = sum_{b, h', c} g_pre[b, co, h', c]                                         (un-rounded)
 * fp32 accumulation of exact products, a padding row stays zero, no scaling: the arithmetic and the kernels of
 * fv_conv1d_weight_grad_dilated_bf16.  On the flat axis q = h' period + c a period conv is a 1-D conv: stride 1 (any
 * Cout, conv_post's 1 included) IS that entry on the views [B, C, H period] with dil = period and zero padding
 * (k - 1) / 2 period; stride 2 and 3 read position stride (q - q mod period) + q mod period + (j - (k - 1) / 2) period
 * and run for the shapes the fp32 entry sends to its matrix-core kernel, Cout >= 64 with Cin k >= 64 -- any other
 * strided shape returns FV_ERR_UNSUPPORTED (DiscriminatorP has none; the fp32 entry takes them).  Units of 64 flat
 * positions; S a function of the shape alone, identical calls return identical bits, the workspace's contents do not
 * matter, no atomics, no waiting between workgroups.  Whatever fv_period_conv_weight_grad refuses is refused with the
 * same code; a map of 2^30 words and more returns FV_ERR_INVALID_ARG.  Two launches.
 */
int64_t fv_period_conv_weight_grad_bf16_workspace_bytes(int B, int Cin, int Cout, int H, int period, int k, int stride);
int fv_period_conv_weight_grad_bf16(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout,
                                    int H, int period, int k, int stride, void* workspace, size_t workspace_bytes,
                                    void* stream);

/*
 * The head of Basis-MelGAN for training (model/generator/basis_melgan.py:140-162 under bin/train.py:64-95, and the
 * weight term of loss.py:39-40); additions of ABI 18, no existing entry changes.  The trunk runs ONCE over B + 1 rows,
 * the last one the response to the all-zero mel, and ends in the raw Y [B+1, C, F]; the reference's second pass and
 * its two differences are rows of one tensor.  Exact fp32, no atomics, workgroups never wait on each other, identical
 * calls return identical bits.  L is the basis length (hop = L/2), basis [L, C] the Linear's weight as it lies in
 * memory.  Every entry checks its arguments before it touches a pointer: B, C or F < 1, L odd or < 2, a null tensor or
 * a result aliasing an input return FV_ERR_INVALID_ARG; L > 256, B > 65535 or more than 2^40 elements
 * FV_ERR_UNSUPPORTED.
 *
 * fv_basis_head_forward:  D[b, c, f] = relu(Y[b, c, f]) - relu(Y[B, c, f]),  D [B, C, F].  The module's weight is D
 *     transposed (a view); its est is fv_basis_ola(D) cut to F hop samples, by linearity of the overlap-add.
 * fv_basis_head_grad:     the adjoint of the whole head in one launch.  g_est [B, F hop] or NULL, g_w [B, C, F] (the
 *     cotangent of weight in D's storage) or NULL, not both NULL;
 *         g_post[b, c, f] = sum_{j < L, f hop + j < F hop} basis[j, c] g_est[b, f hop + j]  +  g_w[b, c, f]
 *         g_Y[b, c, f]    = [Y[b, c, f] > 0] g_post[b, c, f]                                  (b < B)
 *         g_Y[B, c, f]    = -[Y[B, c, f] > 0] sum_{b < B} g_post[b, c, f]
 *     g_Y [B+1, C, F], all of it written.  The taps of the last frame that fall behind the crop get nothing.  An element
 *     is one j-ordered fmaf chain; the batch sum is formed in ascending b by the one block that owns the element.
 * fv_basis_weight_l1:     out[0] = mean |D[b, c, f] - target[b, f, c]|, out[1] = mean D (the reference's
 *     weight_average_value, train.py:73-75); target [B, F, C] in the reference's data layout, out two floats of device
 *     memory.  One reduction launch (per block two doubles in `workspace`) and a one-block finish that adds them in
 *     ascending order.  workspace: at least fv_basis_weight_l1_workspace_bytes(B, C, F) bytes, 8-byte aligned.
 * fv_basis_weight_l1_grad: g[b, c, f] = coef sign(D[b, c, f] - target[b, f, c]) / (B F C), sign(0) = 0, in D's storage
 *     so that fv_basis_head_grad reads it as g_w.  coef: ONE float of device memory, or NULL for 1.
 */
int fv_basis_head_forward(const float* Y, float* D, int B, int C, int F, void* stream);
int fv_basis_head_grad(const float* g_est, const float* g_w, const float* Y, const float* basis, float* g_Y, int B, int C,
                       int F, int L, void* stream);
int64_t fv_basis_weight_l1_workspace_bytes(int B, int C, int F);
int fv_basis_weight_l1(const float* D, const float* target, float* out, int B, int C, int F, void* workspace,
                       size_t workspace_bytes, void* stream);
int fv_basis_weight_l1_grad(const float* D, const float* target, const float* coef, float* g, int B, int C, int F,
                            void* stream);

/*
 * Learning the basis itself: Conv-TasNet's encoder / decoder pair with no separator in between, which produces the
 * basis_signal_weight.npy and weight/ files that Basis-MelGAN trains against; additions of ABI 18, no existing entry
 * changes.  hop = L / 2, F = ceil(n / hop).  The decoder is fv_pack_basis + fv_basis_ola, cut to F hop samples.  Exact
 * fp32 on the fp32 matrix instructions, no atomics, workgroups never wait on each other, identical calls return
 * identical bits.  Every entry checks its arguments before it touches a pointer: B, n or C < 1, L odd or < 2, a null
 * tensor or a result aliasing an input return FV_ERR_INVALID_ARG; L > 256, B > 65535, F >= 2^31 or more than 2^40
 * elements FV_ERR_UNSUPPORTED.  All offsets are 64-bit.
 *
 * fv_basis_encode:     W[b, c, f] = relu(sum_{j < L} enc[c, j] wav[b, f hop + j]), samples at or beyond n read as 0.
 *     wav [B, n], enc [C, L] (a Conv1d(1, C, L, stride = hop, bias = False) weight as it lies in memory), W [B, C, F]:
 *     the trunk's native layout, whose transposed view is the generator's weight [B, F, C].  One launch.
 * fv_basis_learn_grad: the adjoint of est = crop(overlap_add(basis W)) and of the encoder, from g_est [B, F hop]:
 *         G[j, f]       = g_est[b, f hop + j], 0 at or beyond F hop (the taps behind the crop get nothing)
 *         gW[c, f]      = [W[b, c, f] > 0] sum_j basis[j, c] G[j, f]               (registers and LDS only)
 *         d_basis[j, c] = sum_{b, f} G[j, f] W[b, c, f]                             [L, C]
 *         d_enc[c, j]   = sum_{b, f} gW[c, f] wav[b, f hop + j]                     [C, L]
 *     d_enc or d_basis may be NULL (a frozen parameter: its GEMM is not run), not both.  One launch writes S records
 *     (S a function of the shape alone), a combine launch adds them in ascending order.  workspace: at least
 *     fv_basis_learn_grad_workspace_bytes(B, n, C, L) bytes, 4-byte aligned; its contents on entry do not matter.
 */
int fv_basis_encode(const float* wav, const float* enc, float* W, int B, int64_t n, int C, int L, void* stream);
int64_t fv_basis_learn_grad_workspace_bytes(int B, int64_t n, int C, int L);
int fv_basis_learn_grad(const float* wav, const float* g_est, const float* W, const float* basis, float* d_enc,
                        float* d_basis, int B, int64_t n, int C, int L, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * Gradient clipping and the Adam update of a whole parameter set (nn.utils.clip_grad_norm_ + Adam.step() of
 * bin/train.py:126-136 and 176-186; the reference names the fused form itself, apex.optimizers.FusedAdam,
 * train.py:338); additions of ABI 18, no existing entry changes.  Three launches for any number of tensors, exact fp32
 * per element, no atomics, workgroups never wait on each other, identical calls return identical bits.
 *
 * Both entries read one table in DEVICE memory (8-byte aligned): n_tensors rows of fv_adam_tensor and n_chunks
 * entries of fv_adam_chunk that cut every row into pieces of FV_ADAM_CHUNK elements -- row t of n elements owns the
 * entries (t, 0) .. (t, (n - 1) / FV_ADAM_CHUNK), in any order; one workgroup handles one entry.  An entry whose row
 * index lies outside the table is skipped.  All tensors are fp32 and contiguous, of n >= 1 elements; 16-byte loads
 * and stores are used for a row whose pointers are all 16-byte aligned, 4-byte ones otherwise, with the same bits.
 *
 * fv_grad_sq_norm: the 2-norm of all the rows' gradients taken together and clip_grad_norm_'s factor,
 *     out[0] = norm = sqrt(sum_t sum_i g_t[i]^2),     out[1] = coef = min(1, max_norm / (norm + 1e-6))
 * (a NaN norm gives a NaN coef, as torch.clamp passes it).  Launch 1 writes one partial sum of squares per chunk (a
 * double) to `workspace`, launch 2 -- one workgroup -- adds them in ascending order (256 consecutive ranges each in
 * ascending order, then the 256 range sums in ascending order).  workspace: device memory of at
 * least fv_grad_sq_norm_workspace_bytes(n_chunks) bytes, 8-byte aligned; its contents on entry do not matter.  out: two
 * floats of device memory.  Only the g and n fields of a row are read.
 *
 * fv_adam_step: one launch.  With g' = coef[0] g (coef: ONE float of device memory, e.g. out + 1 of fv_grad_sq_norm,
 * or NULL for g' = g),
 *     m = beta1 m + (1 - beta1) g',    v = beta2 v + (1 - beta2) g'^2,
 *     p = p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))
 * per element, where step_size = lr / (1 - beta1^step) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step) are fields of the
 * row, so that rows may be at different step counts; with a coef, g' is written back to g (the gradient holds the
 * clipped values afterwards, as after clip_grad_norm_).  Nothing is read on the host.
 *
 * A null table, counts below 1, n_chunks >= 2^31, a misaligned table, workspace or result, max_norm < 0 (or NaN), or
 * betas outside [0, 1) return FV_ERR_INVALID_ARG, a small workspace FV_ERR_WORKSPACE.
 */
#define FV_ADAM_CHUNK 4096
typedef struct fv_adam_tensor {
    float* p;            /* the parameter */
    float* g;            /* its gradient */
    float* m;            /* exp_avg */
    float* v;            /* exp_avg_sq */
    int64_t n;           /* elements of each */
    float step_size;     /* lr / (1 - beta1^step) */
    float inv_sqrt_bc2;  /* 1 / sqrt(1 - beta2^step) */
} fv_adam_tensor;        /* 48 bytes */
typedef struct fv_adam_chunk {
    int32_t tensor;      /* row of the table */
    int32_t index;       /* which FV_ADAM_CHUNK elements of it */
} fv_adam_chunk;
int64_t fv_grad_sq_norm_workspace_bytes(int64_t n_chunks);
int fv_grad_sq_norm(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                    float max_norm, void* workspace, size_t workspace_bytes, float* out, void* stream);
int fv_adam_step(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                 const float* coef, double beta1, double beta2, double eps, void* stream);

/*
 * fv_grad_bucket_pack (data-parallel training; an addition under ABI 18, no existing entry changes): one launch over the
 * same table copies every gradient into its span of a flat fp32 bucket, times `scale` (1 / world size), so that ONE
 * collective over the bucket averages all gradients and fv_grad_sq_norm / fv_adam_step then read them from the same rows.
 * tensors[r].g is the DESTINATION, row r's span inside the bucket; src[r] (an array of n_tensors pointers in device
 * memory, 8-byte aligned) is the parameter's own gradient, n elements, or NULL for a span of zeros.  A span starts on a
 * 16-byte boundary and is n rounded up to a multiple of 4 floats; the words past n are written as +0, so every word of
 * a bucket laid out this way is written by the launch, whatever it held before.  Element i becomes scale * src[r][i],
 * one fp32 rounding.  A source that is 16-byte aligned is read with 16-byte loads, any other with 4-byte loads of the
 * same elements; the bits do not depend on it.  src[r] == tensors[r].g scales in place.  Only the g and n fields of a
 * row are read; an entry whose row lies outside the table is skipped; no atomics.  A null or misaligned table or
 * pointer array returns FV_ERR_INVALID_ARG.
 */
int fv_grad_bucket_pack(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                        const float* const* src, float scale, void* stream);

/* ------------------------------------------------------------------ *
 * whole-generator plans: an op list replayed over a caller-owned arena
 * ------------------------------------------------------------------ */

typedef struct fv_plan fv_plan_t;

/* tensor slots inside a plan: FV_SLOT_IN is the caller's mel [B,Cin0,T],
 * FV_SLOT_OUT the caller's output, slots >= FV_SLOT_TMP0 live in the workspace */
#define FV_SLOT_NONE (-1)
#define FV_SLOT_IN 0
#define FV_SLOT_OUT 1
#define FV_SLOT_TMP0 2
#define FV_MAX_SLOTS 32
/* caller-provided auxiliary tensors of fv_plan_run_aux: two read-only inputs (output offsets) and a second
 * output; temporaries live in [FV_SLOT_TMP0, FV_SLOT_AUX_IN0) */
#define FV_SLOT_AUX_IN0 28
#define FV_SLOT_AUX_IN1 29
#define FV_SLOT_OUT2 30

fv_plan_t* fv_plan_create(int in_channels);
void fv_plan_destroy(fv_plan_t* plan);

/* append ops; argument meaning as in the fused operators above, tensors named
 * by slot.  Weight pointers are captured, not copied. */
int fv_plan_add_conv1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot,
                       int res_slot, int acc_slot, int acc2_slot, const float* packed,
                       const float* bias, int Cin, int Cout, int k, int dil, int pad,
                       int pad_mode, float pre_slope, float out_div, int post,
                       float act_slope);
int fv_plan_add_conv_transpose1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot,
                                 const float* packed, const float* bias, int Cin, int Cout,
                                 int k, int stride, int pad, int out_pad, float pre_slope,
                                 int post, float act_slope);
int fv_plan_add_conv1d_2src(fv_plan_t* plan, int x_slot, int x2_slot, int y_slot, int y_act_slot,
                            int res_slot, const float* packed, const float* bias, int Cin1,
                            int Cin2, int Cout, int post, float act_slope);
int fv_plan_add_conv1x1_2src_split_f16(fv_plan_t* plan, int x_slot, int x2_slot, int y_slot, int y_act_slot, int res_slot,
                                       const float* packed, const float* bias, int C, float pre_slope, int post,
                                       float act_slope);
int fv_plan_add_residual_stack_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed,
                                         const float* bias_dilated, const float* bias_out, int C, int k, int dil, float slope,
                                         int pad_mode, int post, float act_slope);
/* The residual stack recorded last (256 channels) also carries its two-launch form -- packed_dilated: fv_pack_pair_weight_ex
 * (FV_PAIR_SPLIT_F16) of the dilated conv, packed_pair: fv_pack_conv1x1_2src_split_f16 of (stack[4], skip_layer), hidden_slot:
 * scratch for the hidden tensor -- and a run picks by size (fv_tuning_set "stack_items": tiles per CU, in tenths, up to
 * which the one-launch kernel runs; default: always -- it measured faster at every batch size; 0: never).  Identical bits
 * either way: the switch exists for A/B runs and tests. */
int fv_plan_set_stack_two_launch(fv_plan_t* plan, int hidden_slot, const float* packed_dilated, const float* packed_pair);
/*
 * y = act( ( sum_{j<3} ( conv1d(x_j; w_j, k_j taps, 'same' zero padding) + res_j ) + bias_sum ) / out_div )
 *
 * The MRF merge of a HiFi-GAN stage (hifigan.py:97-103 with modules.py:226-229): the last convs of
 * the three ResBlocks (taps 11 / 7 / 3 in any order, undilated, C -> C) accumulate into one
 * output tile in ONE launch; bias_sum = b_0 + b_1 + b_2.  The three partial results are summed
 * inside the fp32 accumulator rather than as ((r0 + r1) + r2): equal up to fp32 rounding of
 * the additions (the conv1d ops with acc / acc2 keep the reference's association exactly).
 * x_slots / res_slots / packed / k: arrays of 3.  When the layer has too few tiles for one launch
 * to fill the GPU (utterance-length dependent, never batch dependent) the op runs as two launches
 * instead -- members 1 and 2 into the two [B,C,T] scratch slots tmp_slots[0..1], then member 0
 * with both as running-sum inputs; same sum.
 */
int fv_plan_add_conv1d_sum3(fv_plan_t* plan, const int* x_slots, const int* res_slots,
                            const int* tmp_slots, int y_slot, int y_act_slot,
                            const float* const* packed, const float* bias_sum, int C, const int* k,
                            float out_div, int post, float act_slope);
/* fv_resblock1_fused / fv_mrf_stage as plan ops.  Consecutive resblock-pair ops appended under the same
 * non-zero group id (fv_plan_set_group) with equal C, dilation and slopes run as ONE launch. */
int fv_plan_add_resblock_pair(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed1,
                              const float* packed2, const float* bias1, const float* bias2, int C, int k, int dil,
                              float slope, float act_slope);
/* fv_resblock1_fused_ex as a plan op (add1_slot / add2_slot: FV_SLOT_NONE or [B,C,T] slots; mid_slot: a scratch
 * slot, needed at C >= 64 with FV_PAIR_SPLIT_F16, FV_SLOT_NONE otherwise) */
int fv_plan_add_resblock_pair_ex(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, int mid_slot, int add1_slot,
                                 int add2_slot, const float* packed1, const float* packed2, const float* bias1,
                                 const float* bias2, int C, int k, int dil, float slope, float out_div, int post,
                                 float act_slope, int prec);
/* The last pair of a HiFi-GAN with conv_post folded in (hifigan.py:97-106): applies to the op appended last, which must
 * be an ungrouped 16-channel FV_PAIR_SPLIT_F16 pair (with or without add1 / add2).  The pair's own output x' is never
 * stored; the op's output becomes
 *     y[B, 1, T] = post( conv1d( lrelu( x' / out_div, act_slope ); w [1, 16, 7], zero padding 3 ) + bias ),
 * computed on the activated tile in LDS (tiles overlap by the conv's 3-sample halo).  One launch and a [B,16,T]
 * round trip less than the pair followed by fv_conv1d_fused. */
int fv_plan_set_pair_output_conv(fv_plan_t* plan, const float* w, const float* bias, int y_slot, float act_slope, int post);
/* fv_mrf_stage_split_f16 as a plan op (y_act_slot may be FV_SLOT_NONE; workspace: as there, owned by the caller for the
 * plan's lifetime, one per op).  fv_plan_set_pair_output_conv (w [1, C, 7]: 16 or 32 channels here) also applies to this
 * op when it was appended last (the stage's own y is then not stored; y_slot receives the folded conv's [B, 1, T]). */
int fv_plan_add_mrf_stage_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed, int C,
                                    const int* k, const int* dil, float slope, float out_div, int post, float act_slope,
                                    void* workspace, int64_t workspace_bytes);
/* fv_mrf_stage_classes_f16 as a plan op: ys_slot receives r_0 + r_1, yr2_slot r_2 (workspace: as above). */
int fv_plan_add_mrf_stage_classes_f16(fv_plan_t* plan, int x_slot, int ys_slot, int yr2_slot, const float* packed, int C,
                                      const int* k, const int* dil, float slope, void* workspace, int64_t workspace_bytes);
/* fv_conv1d_split_f16 as a plan op; consecutive ops under one non-zero group id with equal C, dilation, padding
 * mode, slopes, out_div and post run as ONE launch */
int fv_plan_add_conv1d_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, int res_slot, int add1_slot,
                                 int add2_slot, const float* packed, const float* bias, int C, int k, int dil,
                                 int pad_mode, float pre_slope, float out_div, int post, float act_slope);
/* fv_conv_transpose1d_split_f16 as a plan op */
int fv_plan_add_conv_transpose1d_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed,
                                           const float* bias, int Cin, int Cout, int k, int stride, int pad,
                                           int out_pad, float pre_slope, float act_slope);
/* The input of the split-f16 transposed conv just added becomes ((x + add1) + add2) / div, formed on chip while its window
 * is loaded (add2_slot may be FV_SLOT_NONE; slots shaped like x).  This is the MRF merge of reference hifigan.py:99-103 --
 * xs = r0; xs += r1; xs += r2; x = xs / num_kernels, in that association -- moved from the end of a stage into the upsampler
 * behind it, so that the stage's last pair position is ONE launch of its three ResBlocks (each storing its r_j) instead of
 * two launches.  The values are formed exactly as the stage-end launch forms them: identical bits. */
int fv_plan_set_input_merge(fv_plan_t* plan, int add1_slot, int add2_slot, float div);
int fv_plan_add_mrf_sum(fv_plan_t* plan, const int* x_slots, int y_slot, int y_act_slot,
                        const float* const* packed1, const float* const* packed2, const float* const* bias1,
                        const float* const* bias2, int C, const int* k, int dil, float slope, float out_div,
                        int post, float act_slope);
int fv_plan_add_upsample_conv1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot,
                                const float* packed, const float* bias, int Cin, int Cout,
                                int k, int rate, int pad, float pre_slope, int post,
                                float act_slope);
int fv_plan_add_pqmf_synthesis(fv_plan_t* plan, int x_slot, int y_slot, const float* h,
                               int S, int ntaps);
/* fv_conv_post_pqmf as a plan op: y_slot receives the FULL-BAND signal [B, 1, S * T']; may carry an output offset
 * (fv_plan_set_output_offset) like the pqmf op */
int fv_plan_add_conv_post_pqmf(fv_plan_t* plan, int x_slot, int y_slot, const float* packed, const float* bias, int Cin,
                               int S, int k, int pad, float pre_slope, int post, const float* h, int ntaps);

/*
 * Bias removal in the epilogue (bin/synthesize.py:74-80 est - generator(0); basis_melgan.py:147-159
 * (est - zero_est, weight - zero_weight); bin/test.py:82-91 est - pattern): the op appended LAST (a conv1d,
 * conv_transpose1d / upsample conv or the pqmf synthesis) subtracts the auxiliary input `aux_slot`
 * (FV_SLOT_AUX_IN0/1, given to fv_plan_run_aux: the cached zero-input response, [C,T'] or [B,C,T']) after its
 * post op / activation.  With y2_slot != FV_SLOT_NONE the op keeps y raw and writes y2 = y - aux (y2 may be
 * FV_SLOT_OUT2 or a temporary); otherwise y itself becomes y - aux.
 */
int fv_plan_set_output_offset(fv_plan_t* plan, int aux_slot, int y2_slot);

/* Association of the MRF running sum in the epilogue of the conv1d ops added from now on:
 * 0 (default)  y = ((acc + acc2) + own) / out_div   -- the LAST ResBlock's conv carries the sum
 * 1            y = ((own + acc) + acc2) / out_div   -- the FIRST ResBlock's conv carries it
 * (own = conv + bias + res).  Both reproduce xs = r0; xs += r1; xs += r2 (hifigan.py:99-102)
 * bit for bit; 1 lets the two large-kernel blocks finish as one grouped launch while the
 * cheapest (3-tap) conv forms the sum. */
int fv_plan_set_sum_order(fv_plan_t* plan, int own_first);

/* Grouping: consecutive conv1d ops appended under the same non-zero group id are
 * declared mutually independent by the caller.  When they are the 11/7/3-tap
 * convolutions at one position of the three ResBlocks of an MRF stage (same
 * shapes, dilation and activation state) the executor runs them as ONE launch
 * (blockIdx.z selects the problem); otherwise one launch each.  0 ends a group. */
int fv_plan_set_group(fv_plan_t* plan, int group);

/* shape inference for a (B, T) call: channels / length of the output tensor
 * and the workspace the plan needs (bytes) */
int fv_plan_output_shape(fv_plan_t* plan, int T, int* out_channels, int64_t* out_len);
int fv_plan_slot_shape(fv_plan_t* plan, int T, int slot, int* channels, int64_t* len);
int64_t fv_plan_workspace_bytes(fv_plan_t* plan, int B, int T);

/* enqueue the whole op list: in [B,Cin0,T] -> out [B,Cout,Tout] */
int fv_plan_run(fv_plan_t* plan, int B, int T, const float* in, float* out,
                void* workspace, int64_t workspace_bytes, void* stream);

/* fv_plan_run with the auxiliary tensors: out2 (FV_SLOT_OUT2; NULL if the plan writes none), aux_in[2]
 * (FV_SLOT_AUX_IN0/1; entries NULL when unused) and aux_batched[2] (non-zero: that input has a batch dimension) */
int fv_plan_run_aux(fv_plan_t* plan, int B, int T, const float* in, float* out, float* out2,
                    const float* const* aux_in, const int* aux_batched, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* The whole-graph entry under the name SURVEY.md section 8(b) lists: the generator forward of a built plan,
 * mel [B,Cin0,T] -> out [B,Cout,Tout] (fv_plan_run; workspace: fv_plan_workspace_bytes(plan, B, T)). */
int fv_generator_run(fv_plan_t* plan, int B, int T, const float* mel, float* out, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* Self-check (tests): the MRF mean's divisor is applied as q0 = v r, q = fma(fma(-d, q0, v), r, q0), r = RN(1 / d) for small
 * integer d (csrc/pair_kernels.hpp div_exact) -- claimed to be the correctly rounded v / d.  Counts, over the fp32 values with
 * bit patterns [first_bits, first_bits + n) and their negatives, where that differs from the device's IEEE division (values
 * whose quotient is not a normal number are skipped); *mismatches (device memory, zeroed by the caller) receives the count. */
int fv_div_probe(unsigned first_bits, int64_t n, float d, unsigned long long* mismatches, void* stream);

/* number of kernel launches one fv_plan_run enqueues */
int fv_plan_num_ops(fv_plan_t* plan);

/*
 * Range guard of a plan's split-f16 launches (FV_PAIR_SPLIT_F16 above: operands must lie inside the f16 range).
 * fv_plan_set_guard: `word` is an int32 in PINNED, DEVICE-MAPPED host memory (hipHostMalloc / torch pin_memory), owned by
 *   the caller and zero-initialised; every split-f16 kernel the plan launches raises FV_GUARD_HIGH in it when one of its final
 *   values is not finite, FV_GUARD_LOW for the low side.  NULL removes the guard.
 * fv_plan_check_range: waits for `stream` (the stream of the plan's last run) to drain, then returns 0 when the word is
 *   clear; otherwise clears it and returns FV_ERR_RANGE (FV_ERR_RANGE_LOW when ONLY the low-side byte is set -- whatever the order the blocks wrote in): the outputs of the run(s) since the last check are not valid
 *   (inf / NaN where the fp32 reference is finite) and must be recomputed on a plan built with FV_PAIR_F32 arithmetic --
 *   fastvocoder_amd/generator/engine.py does that automatically (NativeModule.range_guard).
 */
int fv_plan_set_guard(fv_plan_t* plan, int* word);
int fv_plan_check_range(fv_plan_t* plan, void* stream);

/*
 * Test / tuning hook, not product configuration: sets one of the launchers' tuning switches (csrc/fv_internal.h struct
 * Tuning: "convh_blocks", "pair_blocks", "sched", "sched_switch", "sum3_min", ...) for the whole process.  The launch
 * path reads no environment variable; a process started with FV_TUNING=1 reads FV_<KEY> once at its first launch.
 */
int fv_tuning_set(const char* key, int value);
/*
 * Test hook, host only (no device is touched): the block schedule a fused-pair / split-f16 conv launch of n_members (1 .. 3)
 * members with n_items[m] items of cost[m] each hands to its nblk persistent blocks (csrc/convh_launch.hip) -- the
 * tables the kernels index with blockIdx, as the CPU suite checks them (every item to exactly one block, shares in
 * order, the makespan bound).  The reference has no counterpart: it leaves the partition to ATen.
 *   mode 0: pair_schedule -- longest-processing-time-first over indivisible items for launches with few items per block
 *           (three_members != 0: three-member launches are scheduled too, as the 128-channel launcher asks);
 *   mode 1: pair_cut_schedule -- the contiguous cost-balanced cut, shares 0 .. nblk - 1 (nblk <= 512).
 * table: 512 words.  Returns what the kernel would see as sched_on: 1 -- two words per block, member m's items
 * [lo, lo + count) as lo (11 bits) | count (5 bits) << 11, word 0 = member 0 | member 1 << 16, word 1 = member 2;
 * 2 -- table[i] = first item of share i in the members' concatenated item sequence; 0 -- no table for this shape (the
 * kernel cuts by arithmetic); or a negative FV_ERR_* code.
 */
int fv_debug_pair_schedule(int n_members, const int* n_items, const int* cost, int nblk, int mode, int three_members,
                           unsigned* table);
/*
 * Test and policy hook, host only: the tile widths the fused 128-channel pair launcher (csrc/convh_launch.hip
 * pair_width_plan) picks on its narrow tiles for B utterances of T columns, n_members (1 .. 3) members of taps[m] taps
 * (3, 7 or 11, largest first) and at most `blocks` persistent blocks -- the 11-tap member on 64 or 80 intermediate columns,
 * whichever the block schedule's model finishes earlier (fv_tuning_set "convq_nm11": 64 / 80 force one, -1 chooses).
 * C: 128; dil: 1, 3 or 5 (the choice does not depend on it).
 * info: 12 words -- [0..2] intermediate columns per tile of each member, [3..5] its items, [6..8] the cost of one of its
 * tiles in the schedule's units, [9] the modelled makespan (member switches included; -1: this shape has no block
 * schedule and keeps 64), [10] persistent blocks, [11] 0.  Returns 0 or a negative FV_ERR_* code.
 */
int fv_debug_pair_widths(int C, int B, int T, int dil, int n_members, const int* taps, int blocks, int64_t* info);
/*
 * Test and policy hook, host only: what the 32-channel stage's launchers do with B utterances of T columns on at most nblk
 * (1 .. 256) blocks (csrc/mrfh_launch.hip mrf_class_plan) -- the table the two-class kernel indexes with blockIdx.
 *   force != 0: the split whenever it exists (nblk >= 2 B: what fv_mrf_stage_classes_f16 launches); 0: the split only where
 *   its makespan is below the all-in-one form's (what the generators' policy asks).
 * info[12] = {split (1 / 0: all-in-one), n_A, n_B, makespan, makespan of the all-in-one form, reach of class A, of class B,
 * window columns W, cost of a class-A window, of a class-B window, of an all-in-one window (fv_tuning_set mrf_cost_a /
 * mrf_cost_b / mrf_cost_one, hundreds of cycles; makespans in the same unit), 0}; table[512]: block i (class A first) owns
 * the global columns [table[2 i], table[2 i + 1]) of the B utterances concatenated.  A run's first window is final for
 * W - 2 reach columns, every further one for W - reach.  split = 0: n_A = 0, n_B = nblk, reach of class B = the stage's,
 * the table holds the all-in-one kernel's equal shares.  Returns 0 or a negative FV_ERR_* code.
 */
int fv_debug_mrf_class_schedule(int B, int T, int nblk, int force, int64_t* info, unsigned* table);
/*
 * Timing hook (tools/stage32_bench.py: what a window of one class costs): fv_mrf_stage_classes_f16's launch with the blocks
 * of ONE class of the same table alone -- cls = 1: class A, y = r_2; cls = 2: class B, y = r_0 + r_1.  No guard word.
 */
int fv_debug_mrf_stage_class_f16(const float* x, const float* packed, float* y, int cls, int B, int C, int T, const int* k,
                                 const int* dil, float slope, void* workspace, int64_t workspace_bytes, void* stream);
/*
 * Test hook, host only: the launch log.  Every kernel launch of the library goes through one helper (csrc/fv_internal.h
 * FV_KERNEL_LAUNCH); while the log is on, the helper counts the kernel's host handle in a process-wide table (first-seen
 * order, guarded by a mutex), so that a test can assert WHICH kernel instantiation produced the numbers it compared.  Off,
 * which is the default, a launch pays one relaxed atomic load; on or off, no launch parameter changes and nothing is added
 * on the device.
 *   fv_debug_launch_log(1) clears the table and starts recording, (0) stops (the table stays readable).
 *   fv_debug_launch_log_read writes one line "count<TAB>name<NL>" per kernel into buf (at most cap bytes, no terminator) and
 *   returns the bytes the whole text needs: call with (NULL, 0) first.  Names come from dladdr on the handle and
 *   __cxa_demangle, without return type, "fv::" and argument list: "convh_kernel<2, 2, 1>".
 *   fv_debug_kernel_name gives the same name for a dynamic symbol of the library (a kernel handle or its host stub, whose
 *   "__device_stub__" goes too): what tools/kernel_census.py lists the built instantiations with.  Returns the bytes needed.
 *   fv_debug_launch_log_streams: the helper also counts every launch under its STREAM handle, and so do the helpers of the
 *   library's asynchronous memsets and copies (memset_async / memcpy_async; no other enqueueing call exists in csrc/).
 *   Writes the distinct handles (NULL stream: 0) and their counts, first-seen order, into handles[cap] / counts[cap] (either
 *   may be NULL), the number of asynchronous memsets and copies among them into *copies (may be NULL), and returns the
 *   number of distinct streams: call with cap = 0 first.  Sum of counts = kernel launches of fv_debug_launch_log_read + *copies.
 */
int fv_debug_launch_log(int on);
int64_t fv_debug_launch_log_read(char* buf, int64_t cap);
int64_t fv_debug_launch_log_streams(uint64_t* handles, int64_t* counts, int64_t cap, int64_t* copies);
int64_t fv_debug_kernel_name(const char* symbol, char* buf, int64_t cap);

/* ------------------------------------------------------------------ *
 * measurement hook (bench.py): per-launch timing of the dominant kernel
 * with HIP events recorded on the caller's stream
 * ------------------------------------------------------------------ */
/* When enabled, every conv kernel launch is followed by a hipEvent on its
 * stream (and the first one preceded by one); a launch's time runs from the
 * end of the launch before it to its own end.  fv_profile_collect()
 * synchronises and returns the accumulated (launches, milliseconds,
 * algorithmic flops, algorithmic bytes) of one kernel family and removes
 * those records.  kind: FV_KERNEL_* or -1 for all. */
#define FV_KERNEL_CONV_MFMA32 0 /* 32x32x2 fp32-MFMA implicit-GEMM conv (M > 16 rows) */
#define FV_KERNEL_CONV_MFMA16 1 /* 16x16x4 fp32-MFMA implicit-GEMM conv (M <= 16 rows) */
#define FV_KERNEL_CONV_NARROW 2 /* VALU conv for Cout <= 4 */
#define FV_KERNEL_PAIR16 3      /* fused ResBlock pairs / MRF stage end, C = 16 (16x16x4 fp32 MFMA) */
#define FV_KERNEL_PAIR32 4      /* fused ResBlock pairs, C = 32 */
#define FV_KERNEL_PAIRH16 5     /* fused ResBlock pairs, C = 16, split-f16 operands (16x16x32 f16 MFMA) */
#define FV_KERNEL_PAIRH32 6     /* ... C = 32 */
#define FV_KERNEL_CONVH64 7     /* conv1d with split-f16 operands, C = 64 (ResBlock pairs of the wide stages) */
#define FV_KERNEL_CONVH128 8    /* ... C = 128 */
#define FV_KERNEL_CONVT 9       /* transposed conv (kernel = 2 strides) with split-f16 operands (convt_kernel) */
#define FV_KERNEL_CONVG 10      /* two-source 1x1 conv (ResidualStack tail) with split-f16 operands (convg_kernel) */
#define FV_KERNEL_STACK 11      /* MelGAN ResidualStack as one launch, 32 / 64 / 128 channels, split-f16 operands (convk_kernel) */
#define FV_KERNEL_MRF16 12      /* a whole 16-channel MRF stage as one launch, split-f16 operands (mrfh_kernel) */
#define FV_KERNEL_MRF32 13      /* ... 32-channel (mrfw_kernel) */
int fv_profile_enable(int on);
/* what the measurement adds to a launch (subtract it per launch): a launch's duration is measured completion to
 * completion on its stream, from the end event of the launch before it to its own (its dispatch latency included, as
 * in rocprofv3's dispatch durations); the end-event record is one more packet -- a chain of n (null kernel, event)
 * pairs against a chain of n null kernels */
int fv_profile_bracket_cost(void* stream, int n, double* ms_per_bracket);
/* The device's ACHIEVABLE dense f16 matrix rate, for the `roofline` object of bench.py (fractions against the
 * nominal AND the measured peak): `launches` back-to-back launches of a kernel that does nothing but v_mfma_f32_16x16x32_f16 on
 * registers (two blocks of 8 waves per CU, eight independent accumulators per wave, `iters` x 8 MFMAs per wave, operands that
 * differ per lane), timed by events over the LAST half of the launches -- so that with enough of them the figure is the
 * sustained one.  scratch: >= 512 * 2 * (number of CUs) floats of device memory (one value per thread is stored so that the
 * loop cannot be dropped).  *tflops: executed f16 FLOP (16 384 per MFMA) / second / 1e12. */
int fv_profile_mfma_f16_rate(float* scratch, long long scratch_floats, int launches, int iters, void* stream, double* tflops);
int fv_profile_collect(int kind, int64_t* launches, double* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* FASTVOCODER_HIP_H */
