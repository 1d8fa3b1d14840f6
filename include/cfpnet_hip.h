/*
 * libcfpnet_hip.so -- C ABI of the MI355X (gfx950) CFPNet hot path.
 *
 * The reference (denyingmxd/CFPNet) is pure PyTorch: its "operator interface" for this path is
 * the set of torch ops `Deltar.forward` issues (src/models/deltar.py:34-67).  Each entry point
 * below replaces one family of those ops with a hand-written HIP kernel; the comment on every
 * declaration names the reference lines it stands in for.  The host side
 * (cfpnet_amd/engine.py, via ctypes -- see INTEGRATION.md) strings them together.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer; nothing is allocated or freed here
 *   - activations are NHWC ("tokens": [rows = B*H*W][channels]) with an explicit row pitch
 *     `*_ld` in ELEMENTS, so producers can write straight into a channel slice of a wider
 *     (concatenation) buffer; channel counts, pitches and slice offsets are multiples of
 *     8 elements (bf16) / 4 elements (f32) so that every access is a 16-byte vector
 *   - dtype: CFP_F32, CFP_BF16 or CFP_F16 (IEEE half, saturating stores) storage; all arithmetic accumulates in f32
 *   - all calls are asynchronous on `stream` (a hipStream_t), stateless and re-entrant
 *   - return 0 on success, a negative CFP_E* code otherwise; `cfp_last_error()` gives the
 *     message (thread-local).  No C++ exception crosses this boundary.
 */
#ifndef CFPNET_HIP_H
#define CFPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cfp_stream_t; /* hipStream_t */

enum { CFP_OK = 0, CFP_EINVAL = -1, CFP_ESHAPE = -2, CFP_EHIP = -3 };
enum { CFP_F32 = 0, CFP_BF16 = 1, CFP_F16 = 2 };
/* CFP_F32X3: float32 STORAGE with split-precision ("f16x3") matrix math -- accepted where a call plans or packs for that mode
 * (cfp_conv2d_plan, cfp_conv2d_ws_bytes, cfp_se_gate_fold's output format); kernels that do no matrix math take CFP_F32 tensors as they are. */
enum { CFP_F32X3 = 3 };
enum { CFP_TOF_SAMPLE_UNIFORM = 0, CFP_TOF_SAMPLE_ICDF = 1 };   /* sample_point_from_hist_parallel: --sample_uniform / default */
enum { CFP_ACT_NONE = 0, CFP_ACT_RELU = 1, CFP_ACT_LRELU = 2, CFP_ACT_SILU = 3, CFP_ACT_GELU = 4, CFP_ACT_SIGMOID = 5 };

int cfp_version(void);
const char* cfp_last_error(void);

/* Dense convolution / linear layer as an implicit GEMM on the matrix cores:
 *   out[m, n] = act( (sum_k A[m,k] * w[n,k]) * scale[n] + shift[n] ) + residual[m, n]
 * with m = (b, ho, wo), k = (kh, kw, ci), w packed [Cout][KH][KW][Cin].
 * Replaces nn.Conv2d 3x3 / 1x1 (+ folded BatchNorm + activation + skip add):
 *   decoder.py:43-58,70-80 (UpSampleBN, conv0..conv4), decoder.py:13 (depth_head.conv3x3),
 *   transformer.py:197-200,240-244 (DAPM convs), transformer.py:132 (GSA sr conv),
 *   nn.Linear in transformer.py:24-36 / convnext.py:32-34 / encoder.py:10-12 (KH=KW=1, H=1),
 *   and the encoder's conv_stem / conv / conv_exp / conv_pw / conv_pwl (encoder.py:57-69).
 * scale/shift may be NULL (1 / 0).  residual may be NULL.  Cin % 8 == 0 (bf16) or % 4 (f32). */
int cfp_conv2d_nhwc(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                    const void* residual, int res_ld, void* out, int out_ld,
                    int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad_t, int pad_l, int Ho, int Wo, int act, int dtype,
                    void* ws, size_t ws_bytes, cfp_stream_t stream);

/* cfp_conv2d_nhwc with two more fusions (same reference ops, fewer launches):
 *   - ln_gamma/ln_beta != NULL: LayerNorm over the Cout axis (eps = ln_eps) applied after
 *     scale/shift/act, the residual is added AFTER the LayerNorm:
 *         out = LN(act(conv * scale + shift)) * gamma + beta + residual
 *     (transformer.py:63,68-70: merge -> norm1, mlp -> norm2 -> + x).  Fused into the GEMM
 *     epilogue when a tile spans exactly Cout channels (bf16, Cout in {16,32,64,128}), otherwise
 *     run as a second kernel on `out` in place.  CFP_CONV_X3 launches whose K is split run it inside
 *     the finishing sum of the splits (Cout / 4 a power of two <= 64; round 5).
 *   - per_image_weights != 0: `w` holds B weight matrices [B][Cout][K]; image b of the batch uses
 *     matrix b.  Used for the squeeze-excite gate folded into the project conv of the encoder's
 *     inverted-residual blocks (x * gate[b,:]) @ W^T == x @ (W * gate[b,:])^T, see cfp_se_fold.
 *   - per_image_weights & CFP_CONV_W2 (16-bit pointwise layers with shared weights): TWO-TERM weights.  Every row of `w` is
 *     [hi | lo] with hi = round16(W), lo = round16(W - hi), each half zero-padded to a multiple of 64 elements; the kernel runs
 *     the K loop over both halves against the same activations, so the layer sees its weights with ~22 (fp16) / ~16 (bf16)
 *     significant bits instead of 11 / 8.  Weight rounding of the pointwise layers is 0.8e-3 of the fp16 engine's 0.9e-3
 *     relative-L1 error (profiles/r2_precision_budget.md). */
/*   - per_image_weights & CFP_CONV_X3 (dtype CFP_F32): split-precision matrix math on float32 tensors.  Every value is taken as
 *     hi + lo (two IEEE halves, ~21 significant bits) and the product as A_hi W_hi + A_hi W_lo + A_lo W_hi on
 *     v_mfma_f32_16x16x32_f16 with float32 accumulation: 3/16 of the 16-bit matrix rate instead of the 1/16 of the float32 MFMA,
 *     product error ~2^-21.  `w` is then the PRE-SPLIT operand written by cfp_pack_w_x3 ([Cout][ceil(K/32)][hi(32) | lo(32)] halves;
 *     with CFP_CONV_PER_IMAGE: B such matrices, as cfp_se_gate_fold writes them for dtype CFP_F32X3).  This is the mode whose results
 *     stay inside the reference tolerance (1e-3 relative L1 on the depth map, /root/reference/src/models/deltar.py:34-67 in float32)
 *     for every weight family -- the default of the drop-in boundary. */
enum { CFP_CONV_PER_IMAGE = 1, CFP_CONV_W2 = 2, CFP_CONV_IN_FLIGHT = 4, CFP_CONV_X3 = 8, CFP_CONV_WS_TICKETS = 16 };   /* bits of cfp_conv2d_nhwc_ex's `per_image_weights` argument.
 * CFP_CONV_IN_FLIGHT: a hint -- this launch will run beside launches of other batches (several captured forwards in flight): the tile is then
 * chosen for the resources it holds rather than for its own latency (larger tiles).  Results do not depend on it: every tile walks K in the same order.
 * CFP_CONV_WS_TICKETS (CFP_CONV_X3 launches): the first CFP_CONV_TICKET_BYTES of `ws` are a TICKET AREA -- all zero when the workspace is first handed
 * over, and left all zero by every launch -- and the split-K slabs follow it (ws_bytes >= CFP_CONV_TICKET_BYTES + cfp_conv2d_ws_bytes(...)).  When K is
 * split, the workgroup that reaches an output tile last then finishes it (slabs summed in split order, scale / shift / act / residual), instead of a
 * second launch doing so: one kernel less per split layer, the same bits.  Launches that share a workspace must be ordered (one stream), as they must
 * for the slabs. */
#define CFP_CONV_TICKET_BYTES 4096
int cfp_conv2d_nhwc_ex(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                       const void* residual, int res_ld, void* out, int out_ld,
                       int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                       int pad_t, int pad_l, int Ho, int Wo, int act, int dtype,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, int per_image_weights,
                       void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Weights [rows][K] float32 (K = KH*KW*Cin in (kh, kw, ci) order; rows = Cout, or B*Cout for per-image weights) -> the pre-split
 * operand of the CFP_CONV_X3 kernels: [rows][ceil(K/32)][hi(32) | lo(32)] IEEE halves in the kernels' lane order, zero padded to whole
 * 32-channel K-steps.  cfp_pack_w_x3_elems = halves in that buffer.  Replaces nothing in the reference (a weight re-layout, like the
 * [Cout][KH][KW][Cin] packing of every other mode); the layers are the nn.Conv2d / nn.Linear calls listed at cfp_conv2d_nhwc. */
size_t cfp_pack_w_x3_elems(long long rows, int K);
int cfp_pack_w_x3(const float* w, void* out, long long rows, int K, cfp_stream_t stream);

/* Scratch cfp_conv2d_nhwc wants for (M = B*Ho*Wo, Cout, K = KH*KW*Cin): non-zero only for layers it
 * runs split-K (few output tiles, long K: the GSA sr convs, the 1/32-scale pointwise convs).  With
 * ws == NULL or too small the layer runs un-split (same result up to f32 re-association). */
size_t cfp_conv2d_ws_bytes(int M, int Cout, int K, int dtype);

/* Kernel plan cfp_conv2d_nhwc uses for a problem (per-kernel accounting in bench.py and
 * tools/conv_bench.py).  *variant: 0..3 = first-generation tiles 256x16 / 256x32 / 128x64 /
 * 128x128 (f32); 100 + v = second-generation (bf16, LDS-DMA staged) variant v; 200 + v = direct 3x3
 * (LDS halo tile) variant v; 400 + v = f16x3 implicit-GEMM variant v, 500 = the f16x3 whole-depth-halo 3x3 kernel (dtype CFP_F32X3: float32
 * storage, CFP_CONV_X3); 600 + v = tile v of the 16-bit chunk 3x3 kernel (conv3x3_chunk.hip).  *splits = K-splits.  KH/stride describe the filter (K = KH*KH*Cin);
 * rows_per_batch > 0 describes a per_image_weights call (B images of rows_per_batch rows).
 * The answer is the launch's own decision (one function, csrc/conv_route.hip) for the CANONICAL problem of these arguments: KW = KH, padding 1
 * for a 3x3 filter and 0 otherwise, channel strides equal to the channel counts, B images of M / B output pixels, no LayerNorm, no residual,
 * no moments, a sufficient workspace, launches in flight only under cfp_debug_set(17, 1), and -- for the 16-bit types -- a problem within
 * the second-generation kernel's limits (K <= 16384, operands within 32-bit byte offsets).  300 and 500 are first choices: those two launchers
 * may decline a problem whose halo does not fit the LDS, and the call then runs the implicit GEMM. */
int cfp_conv2d_plan(int M, int Cout, int K, int KH, int stride, int dtype, int rows_per_batch, int B, int* variant,
                    int* splits);

/* The tile of the 16-bit chunk 3x3 kernel (csrc/conv3x3_chunk.hip: stride 1, more than 64 input channels, 64-channel chunks of the input
 * halo through LDS; 0 = 128 channels x 8 x 16 pixels, 1 = 64 channels x 8 x 16 pixels) that cfp_conv2d_nhwc runs for a bf16 / f16
 * 3x3 stride-1 convolution of M = B*Ho*Wo output pixels, or -1 where the problem keeps its implicit GEMM / direct kernel (always for
 * Cin <= 64 or Cin % 8 != 0).  in_flight = graphs replayed side by side: above 1 the answer is the plan of CFP_CONV_IN_FLIGHT calls.
 * cfp_debug_set(0, 600 + v) forces tile v (an error for a problem the kernel does not take); cfp_debug_set(40, 0) switches the kernel off
 * everywhere, 2 runs it wherever it can, 1 is this plan. */
int cfp_conv3x3_chunk_variant(int M, int Cin, int Cout, int in_flight);

/* First-generation tile choice for (M, Cout): 0 = 256x16, 1 = 256x32, 2 = 128x64, 3 = 128x128. */
int cfp_conv2d_variant(int M, int Cout);

/* Test/benchmark knobs, not for production use (process-global, not thread-safe):
 * key 0 = force second-generation variant v, or 200 + v = direct 3x3 variant v (-1 = automatic), key 1 = force K-splits (-1 = automatic),
 * key 2 = 1 routes bf16 through the first-generation kernel; keys 3 / 4 = depthwise 3x3 channel vectors per
 * workgroup (8 / 16) and output rows per strip (0 = automatic); key 5 = 1 forces the VALU depthwise kernel; key 6 = 16-bit depthwise
 * 3x3 kernel (1 or 2, CFP_EINVAL otherwise); keys 7 and 8 are unused (CFP_EINVAL); keys 9-40 are listed in README.md ("Kernel choices")
 * and at the dispatch in csrc/conv_route.hip.  The depthwise keys change the slot counts of cfp_dwconv3x3_strips / _se_parts too. */
int cfp_debug_set(int key, int value);

/* Depthwise 3x3 convolution, stride 1/2, explicit (TF-"SAME", possibly asymmetric) padding, fused
 * BatchNorm scale/shift + activation.  w packed [9][C].  HBM-bandwidth-bound.
 * Replaces timm InvertedResidual.conv_dw + bn2 + SiLU (encoder.py:66-69, 24 convs).
 * Kernels: float32 storage -> dw3x3_rows_kernel (round 5: register-sliding rows, no LDS; csrc/dw3x3_rows.hip), 16-bit storage with
 * C % 16 == 0 -> dw3x3_slide_kernel (diagonal-weight MFMA, csrc/dw3x3_slide.hip), otherwise the LDS-strip kernel of csrc/dwconv.hip.
 * act is one of CFP_ACT_* (CFP_EINVAL otherwise, on all three depthwise 3x3 entry points); the kernel choice does not depend on it. */
int cfp_dwconv3x3_nhwc(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                       void* out, int out_ld, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
                       int Ho, int Wo, int act, int dtype, cfp_stream_t stream);

/* cfp_dwconv3x3_nhwc that ALSO emits sums of the stored output per (image, row strip, channel):
 *   partial[b][s][c] (f32), s < cfp_dwconv3x3_strips(B, Ho, Wo, C, stride, dtype)
 * so the H*W mean that timm's SqueezeExcite takes of this tensor (x.mean((2,3))) needs no extra
 * pass: cfp_se_hidden(partial, nsplit = strips, ...) consumes it directly.  Strip order and the
 * in-strip reduction order are fixed: the sums are run-to-run deterministic. */
int cfp_dwconv3x3_strips(int B, int Ho, int Wo, int C, int stride, int dtype);
/* The number of partial-sum slots per image a cfp_dwconv3x3_sum_nhwc LAUNCH writes for these full arguments, any dtype; 0 when such a
 * launch refuses them (CFP_ESHAPE: the input extent or a row pitch gives another kernel or slot count than cfp_dwconv3x3_strips, which is
 * asked WITHOUT them and sized `partial`).  Host-side only, no GPU work: tests/test_abi.py sweeps shapes and checks that it equals
 * cfp_dwconv3x3_strips (a mismatch was an out-of-bounds write into `partial`, found and fixed in round 5). */
int cfp_dwconv3x3_launch_slots(int B, int H, int W, int Ho, int Wo, int C, int stride, int in_ld, int out_ld, int dtype);
int cfp_dwconv3x3_sum_nhwc(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                           void* out, int out_ld, float* partial, int B, int H, int W, int C, int stride,
                           int pad_t, int pad_l, int Ho, int Wo, int act, int dtype, cfp_stream_t stream);

/* Large-kernel depthwise convolution (odd k <= 31; 7 / 15 / 31 have dedicated kernels), stride 1,
 * "same" padding, fused bias + BatchNorm + ReLU.  w packed [C][kx][ky] as f32 (per-channel
 * contiguous, column-major taps: the kernel slides vertically and fetches weights through the
 * scalar cache).  Vector-FMA-bound.  Replaces Block14.dwconv2 + bn1 + relu (convnext.py:30,45-47). */
int cfp_dwconv_large_nhwc(const void* in, int in_ld, const float* w, const float* scale, const float* shift,
                          void* out, int out_ld, int B, int H, int W, int C, int k, int act, int dtype,
                          cfp_stream_t stream);

/* cfp_dwconv_large_nhwc on the matrix cores (bf16, k in {7, 15, 31}): every kernel row is a banded Toeplitz product,
 * 62 MFMAs per 16x16 output tile of one channel for k = 31.  `toeplitz` holds the bands in MFMA B-operand layout,
 *   toeplitz[c][ky][h][lane][e] = w[c][ky][kx],  kx = 32 h + 8 (lane >> 4) + e - (LM - halo) - (lane & 15)   (0 outside [0, k))
 * with halo = (k-1)/2, LM = halo rounded up to 8, h < NH = ceil((16 + LM + halo) / 32); cfp_dwconv_large_toeplitz_elems
 * gives its size in elements.  It is built once per weight tensor on the host (cfpnet_amd/engine.py). */
size_t cfp_dwconv_large_toeplitz_elems(int C, int k);
/* The same table built on the device from float32 weights [C][k][k] (training: the master weights change every step); flip != 0
 * gives the table of the 180-degree-rotated kernel (the data gradient).  out: cfp_dwconv_large_toeplitz_elems(C, k) 16-bit elements. */
int cfp_dwconv_large_toeplitz(const float* w, void* out, int C, int k, int flip, int dtype, cfp_stream_t stream);
int cfp_dwconv_large_mfma_nhwc(const void* in, int in_ld, const void* toeplitz, const float* scale, const float* shift,
                               void* out, int out_ld, int B, int H, int W, int C, int k, int act, int dtype,
                               cfp_stream_t stream);

/* Per-(batch, channel) sums over H*W, split in `nsplit` row slices: partial[b][s][c] (f32).
 * Consumers divide by H*W.  Replaces x.mean((2,3)) in the SE block and `.mean([2,3])` of
 * DepthRegression (decoder.py:24-25; conv1x1 and mean commute). */
int cfp_channel_sum(const void* in, int in_ld, float* partial, int B, int HW, int C, int nsplit, int dtype,
                    cfp_stream_t stream);

/* Squeeze-excite, first half: mean -> FC(C->R) + bias -> SiLU; hidden[b][r] f32.  w_reduce [R][C] f32.
 * Replaces timm SqueezeExcite.conv_reduce + act (inside the encoder.py:66-69 blocks). */
int cfp_se_hidden(const float* partial, int nsplit, float inv_hw, const float* w_reduce, const float* b_reduce,
                  float* hidden, int B, int C, int R, cfp_stream_t stream);

/* Squeeze-excite, second half, in place: x[b,hw,c] *= sigmoid(hidden[b] . w_expand_t[:, c] + b_expand[c]).
 * w_expand_t is the expand weight TRANSPOSED to [R][C] f32.  Replaces conv_expand + sigmoid gate + multiply. */
int cfp_se_scale(void* x, int ld, const float* hidden, const float* w_expand_t, const float* b_expand,
                 int B, int HW, int C, int R, int dtype, cfp_stream_t stream);

/* Squeeze-excite gate folded into the following project conv's weights:
 *   w_out[b][n][c] = w_proj[n][c] * sigmoid(hidden[b] . w_expand_t[:, c] + b_expand[c])
 * (x * gate[b,:]) @ W^T == x @ (W * gate[b,:])^T, so conv_expand + sigmoid + the gating multiply of
 * SqueezeExcite and conv_pwl become one per-image-weights GEMM (cfp_conv2d_nhwc_ex) with no pass
 * over the expanded activation.  hidden from cfp_se_hidden; w_expand_t [R][C] f32; w_proj [Cout][C]
 * and w_out [B][Cout][C] in `dtype`. */
int cfp_se_fold(const void* w_proj, void* w_out, const float* hidden, const float* w_expand_t, const float* b_expand,
                int B, int Cout, int C, int R, int dtype, cfp_stream_t stream);

/* Front half of a stride-1 inverted-residual block in one launch (csrc/mbconv.hip): conv_pw 1x1 (Cin -> mid) + BN1 + SiLU ->
 * conv_dw 3x3 (depthwise, padding 1) + BN2 + SiLU (timm InvertedResidual as the reference builds it, encoder.py:66-69) + the
 * per-tile channel sums squeeze-excite needs.  The expanded tensor never reaches HBM.
 *   x [B,H,W,x_ld] (Cin channels); wpw [mid][KP + 8] 16-bit with KP = Cin rounded up to 32 (cfp_mbconv_plan), zero padding behind
 *   the Cin real columns: the LDS image layout of the weights; s1 / t1, s2 / t2 [mid] f32: BatchNorm folded to scale / shift;
 *   wdw [9][mid] 16-bit (tap-major, like cfp_dwconv3x3_nhwc); out [B,H,W,out_ld] (mid channels); partial (may be NULL)
 *   [B][tiles_per_image][mid] f32 channel sums per spatial tile (tiles_per_image from cfp_mbconv_plan; feed cfp_se_gate_fold with
 *   nsplit = tiles_per_image).  bf16 / f16 only; Cin % 8 == 0, mid % 16 == 0.  cfp_mbconv_plan returns CFP_ESHAPE if the shape
 *   does not fit (the engine then runs cfp_conv2d_nhwc + cfp_dwconv3x3_sum_nhwc). */
int cfp_mbconv_plan(int B, int H, int W, int Cin, int mid, int* tiles_per_image, int* KP);
int cfp_mbconv_expand_dw(const void* x, int x_ld, const void* wpw, const float* s1, const float* t1, const void* wdw,
                         const float* s2, const float* t2, void* out, int out_ld, float* partial, int B, int H, int W, int Cin,
                         int mid, int dtype, cfp_stream_t stream);

/* A 3x3 convolution and the 1x1 convolution that is its only reader in one launch (csrc/conv3x3_halo.hip, PW = true):
 *   out = act2(scale2 * conv1x1(round16(act1(scale1 * conv3x3(in) + shift1))) + shift2) (+ residual, added to the rounded value).
 * Replaces timm EdgeResidual's conv_exp + bn1 + SiLU + conv_pwl + bn2 (+ shortcut) (encoder.py:57-69, the blocks of stages conv1 / conv2;
 * oracle/cfpnet_oracle.py:85-89) as two cfp_conv2d_nhwc launches; the expanded tensor [B,Ho,Wo,Cmid] never reaches HBM, and the value
 * fed to the 1x1 is bit for bit the one the first launch would have stored, and the 1x1 sums its K blocks in the order of
 * cfp_conv2d_nhwc's kernels into one accumulator: the result is the pair's bit for bit.
 *   in [B,H,W,in_ld] (Cin channels); w1 [Cmid][3*3*Cin] as cfp_conv2d_nhwc lays weights out; w2_pad [16 ceil(Cout / 16)][Kp], Kp = Cmid
 *   rounded up to 32: the [Cout][Cmid] weights with zero rows / columns as padding; scale / shift [Cmid] and [Cout] f32 (may be NULL = 1 / 0);
 *   residual / out [B,Ho,Wo,res_ld / out_ld] (Cout channels; out may be a channel slice of a wider buffer); stride 1 or 2 with
 *   explicit top / left padding as cfp_conv2d_nhwc.  act1 any CFP_ACT_*, act2 CFP_ACT_NONE or CFP_ACT_LRELU (CFP_EINVAL otherwise).
 *   bf16 / f16 only.
 * cfp_conv3x3_pw_fused_variant -> the whole-depth-halo variant (cfp_debug_set(0, 300 + v)) the launch runs for this shape, or -1 when
 * it does not take it: every Cmid channel must live in one workgroup (Cmid <= 224, <= 160 at stride 2; Cout <= 64; channel counts
 * multiples of 8; Cin <= 128; the 1x1 weights within one weight stage; LDS within a CU).  The launch returns CFP_ESHAPE for such a
 * shape: the caller keeps the two launches, nothing falls back silently. */
int cfp_conv3x3_pw_fused_variant(int Cin, int Cmid, int Cout, int stride, int dtype);
int cfp_conv3x3_pw_fused(const void* in, int in_ld, const void* w1, const float* scale1, const float* shift1, int act1,
                         const void* w2_pad, const float* scale2, const float* shift2, int act2, const void* residual, int res_ld,
                         void* out, int out_ld, int B, int H, int W, int Cin, int Cmid, int Cout, int stride, int pad_t, int pad_l,
                         int Ho, int Wo, int dtype, cfp_stream_t stream);

/* Short-K pointwise GEMM (csrc/pw_rows.hip), bf16 / f16:
 *   out[m, n] = act(scale[n] * sum_k in[m, k] * w[n, k] + shift[n]),  m < M, k < K <= 256, n < N.
 * Replaces the conv_pw + bn1 + SiLU of timm's InvertedResidual blocks (encoder.py:57-69; oracle/cfpnet_oracle.py) as a cfp_conv2d_nhwc
 * launch, bit for bit: a workgroup keeps its 64 input rows in registers as whole MFMA fragments and streams only the weights, one group
 * of output columns per workgroup.
 *   in [M][in_ld] (K channels; may be a channel slice of a wider buffer), w [N][K] as cfp_conv2d_nhwc lays out 1x1 weights, scale / shift
 *   [N] f32 (may be NULL = 1 / 0), out [M][out_ld] (N channels; may be a channel slice).  act CFP_ACT_NONE or CFP_ACT_SILU (CFP_EINVAL
 *   otherwise).  groups: column groups of the launch, 0 = chosen for about two workgroups per CU, else clamped to what the shape allows.
 * cfp_pw_rows_fits -> 1 when the launch takes the shape: 16-bit storage, K % 8 == 0 and K <= 256, N % 8 == 0, row pitches multiples of
 * 8 elements that cover K / N, 0 < M < 2^31; else 0, and the launch returns CFP_ESHAPE: the caller keeps cfp_conv2d_nhwc, nothing falls
 * back silently.  cfp_pw_rows_groups -> the column groups an automatic launch runs, *max_groups (may be NULL) = the most it can run. */
int cfp_pw_rows_fits(long long M, int K, int N, int in_ld, int out_ld, int dtype);
int cfp_pw_rows_groups(long long M, int K, int N, int* max_groups);
int cfp_pw_rows(const void* in, int in_ld, const void* w, const float* scale, const float* shift, int act, void* out, int out_ld,
                long long M, int K, int N, int groups, int dtype, cfp_stream_t stream);

/* cfp_se_hidden + cfp_se_fold in one launch (mean -> FC -> SiLU -> FC -> sigmoid -> per-image project weights),
 * structured for latency: this is what the engine calls between the depthwise conv and the project conv of every
 * inverted-residual block.  Same arguments as the two calls it replaces; C <= 2048, R <= 64. */
int cfp_se_gate_fold(const float* partial, int nsplit, float inv_hw, const float* w_reduce, const float* b_reduce,
                     const float* w_expand_t, const float* b_expand, const void* w_proj, void* w_out,
                     int B, int Cout, int C, int R, int dtype, cfp_stream_t stream);

/* cfp_dwconv3x3_nhwc + the squeeze-excite reduce FC applied to the workgroup's channel sums (16-bit storage with C % 16 == 0, or
 * float32 storage -- the default f16x3 mode -- with C % 8 == 0; R <= 64):
 * timm InvertedResidual conv_dw -> bn2 -> act, and of SqueezeExcite (x.mean((2, 3)) -> conv_reduce) the part that is LINEAR in the
 * sums: every workgroup (image b, row strip, channel block) writes
 *   hpart[b][k][r] = sum_{c in block} w_reduce[r][c] * (sum of its stored output pixels of channel c),   k = strip * blocks + block,
 * K = cfp_dwconv3x3_se_parts(...) partials per image (0: shape / dtype not supported).  w_reduce [R][C] f32.  cfp_se_gate_fold2 adds
 * them, scales by 1 / (Ho * Wo) and finishes the block.  Reference: encoder.py:66-69 (timm tf_efficientnetv2_b3 blocks[3..5]). */
int cfp_dwconv3x3_se_parts(int B, int Ho, int Wo, int C, int stride, int dtype);
int cfp_dwconv3x3_se_nhwc(const void* in, int in_ld, const void* w, const float* scale, const float* shift, void* out, int out_ld,
                          const float* w_reduce, int R, float* hpart, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
                          int Ho, int Wo, int act, int dtype, cfp_stream_t stream);

/* The squeeze-excite tail when the depthwise kernel has already applied the reduce FC to its channel sums (the reduce layer is
 * linear in them): hpart [B][K][R] f32 partial dot products (cfp_dwconv3x3_se_nhwc), added in k order;
 *   hidden = silu(inv_hw * sum_k hpart + b_reduce);  gate = sigmoid(hidden . w_expand_t + b_expand);  w_out[b][n][c] = w_proj[n][c] * gate[c]
 * with w_proj the FLOAT32 project weights [Cout][C] (the folded weights are rounded to `dtype` once) and w_out [B][Cout][C] in `dtype`.
 * Replaces timm SqueezeExcite + the gate multiply as cfp_se_gate_fold does; one full-chip launch.  C % 8 == 0, R <= 64. */
int cfp_se_gate_fold2(const float* hpart, int K, float inv_hw, const float* b_reduce, const float* w_expand_t, const float* b_expand,
                      const float* w_proj, void* w_out, int B, int Cout, int C, int R, int dtype, cfp_stream_t stream);

/* x[b, hw, c] *= gate[b, c] in place. */
int cfp_scale_channels(void* x, int ld, const float* gate, int B, int HW, int C, int dtype, cfp_stream_t stream);

/* Row LayerNorm over C with affine, optional residual add afterwards:
 *   out[r,:] = LN(in[r,:]) * gamma + beta (+ residual[r,:])
 * Replaces nn.LayerNorm in transformer.py:38-39,63,68,70 and convnext.py:31,49. */
int cfp_layernorm(const void* in, int in_ld, const float* gamma, const float* beta, float eps,
                  const void* residual, int res_ld, void* out, int out_ld, int rows, int C, int dtype,
                  cfp_stream_t stream);

/* Linear attention, reduction half (attention.py:31-43):  for every key group g and head h
 *   KV[g,h] = sum_s (elu(K_s)+1)^T (V_s / v_length),   Ksum[g,h] = sum_s (elu(K_s)+1)
 * Keys live on an [NB, Hk, Wk] grid (row pitch ld); group (b, gy, gx) owns the th x tw tile
 * clipped to [cy0,cy1) x [cx0,cx1).  With count_pad != 0, tile positions outside the grid count
 * as zero-feature tokens (K = 1, V = 0): the zero-padded windows of transformer.py:101-107.
 * Covers hist2image (tile 1x16), LSA windows, GSA (one tile per batch) and DAPM (inside rectangle).
 * ws: f32 scratch of cfp_attn_kv_ws_floats() floats. */
size_t cfp_attn_kv_ws_floats(int NB, int Hk, int Wk, int th, int tw, int heads, int d);
int cfp_attn_kv_reduce(const void* k, int k_ld, const void* v, int v_ld, float* kv, float* ksum, float* ws,
                       int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                       int count_pad, float v_length, int heads, int d, int dtype, cfp_stream_t stream);

/* cfp_attn_kv_reduce with the clip rectangle and v_length read from DEVICE memory: rec = the int32[9] zone record of
 * cfp_zone_crop (sy, sx, tzh, tzw, y0, y1, x0, x1, n_inside); the clip is [rec.y0,rec.y1) x [rec.x0,rec.x1), the zone_mask
 * rectangle of fusion.py:104, and v_length = max(rec.n_inside, 1) (transformer.py:215-230: DAPM's keys are the inside-zone
 * tokens).  Grid, split count and workspace depend on the tile only, so a captured graph serves every record. */
int cfp_attn_kv_reduce_dev(const void* k, int k_ld, const void* v, int v_ld, float* kv, float* ksum, float* ws,
                           int NB, int Hk, int Wk, int th, int tw, const int* rec, int count_pad, int heads, int d, int dtype,
                           cfp_stream_t stream);

/* cfp_attn_kv_reduce[_dev] on the key TOKENS: the k|v projection runs inside the reduction, K|V = x @ w_kv^T never reaches memory.
 * x: [NB * Hk * Wk][D] tokens (pitch x_ld, a multiple of 8), D = heads * d; w_kv: [2 D][D] in the storage type, rows 0 .. D-1 the
 * k projection, D .. 2D-1 the v projection (a linear layer without bias).  bf16 / f16 only.  kv, ksum and the split slabs in ws are
 * bit-identical to cfp_linear (no scale, shift or activation) followed by cfp_attn_kv_reduce[_dev] on its output; geometry, split count
 * and workspace are cfp_attn_kv_reduce's.  cfp_attn_kv_project_fits: 1 if the launch takes the problem (D in 32 / 64 / 128, heads 4 / 8,
 * a 16-bit dtype, and the rows of one split within the kernel's LDS budget), else 0 -- the launch then refuses it with CFP_ESHAPE
 * (CFP_EINVAL for the dtype) before anything runs, and the caller keeps the pair. */
int cfp_attn_kv_project_fits(int NB, int Hk, int Wk, int th, int tw, int heads, int d, int dtype);
int cfp_attn_kv_project_reduce(const void* x, int x_ld, const void* w_kv, float* kv, float* ksum, float* ws,
                               int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                               int count_pad, float v_length, int heads, int d, int dtype, cfp_stream_t stream);
int cfp_attn_kv_project_reduce_dev(const void* x, int x_ld, const void* w_kv, float* kv, float* ksum, float* ws,
                                   int NB, int Hk, int Wk, int th, int tw, const int* rec, int count_pad, int heads, int d, int dtype,
                                   cfp_stream_t stream);

/* Linear attention, query half (attention.py:48-49):
 *   out[q,h,:] = (Q_q,h . KV[g(q),h]) / (Q_q,h . Ksum[g(q),h] + eps) * v_length,  Q = elu(q)+1
 * Queries live on an [NB, Hq, Wq] grid; g(q) = (b, y / qth, x / qtw).  Queries inside the
 * exclusion rectangle [ey0,ey1) x [ex0,ex1) get 0 (DAPM: only outside-zone tokens receive a
 * message, transformer.py:233-234). */
int cfp_attn_apply(const void* q, int q_ld, const float* kv, const float* ksum, void* out, int out_ld,
                   int NB, int Hq, int Wq, int qth, int qtw, int ey0, int ey1, int ex0, int ex1,
                   float v_length, float eps, int heads, int d, int dtype, cfp_stream_t stream);

/* cfp_attn_apply with the exclusion rectangle [rec.y0,rec.y1) x [rec.x0,rec.x1) and v_length = max(rec.n_inside, 1) read
 * from the device zone record (transformer.py:233-234 with the zone_mask of fusion.py:104), as cfp_attn_kv_reduce_dev. */
int cfp_attn_apply_dev(const void* q, int q_ld, const float* kv, const float* ksum, void* out, int out_ld,
                       int NB, int Hq, int Wq, int qth, int qtw, const int* rec, float eps, int heads, int d, int dtype,
                       cfp_stream_t stream);

/* Fused tail of a LoFTR encoder layer, one launch (bf16 only; D in {32,64,128}, heads in {4,8}):
 *   msg = cfp_attn_apply(q, kv, ksum)                                   attention.py:48-49
 *   y1  = LayerNorm(msg @ w_merge^T; ln1)                               transformer.py:63
 *   h   = relu([x | y1] @ w_mlp0^T)                                     transformer.py:66-67 (mlp.0 + ReLU)
 *   out = LayerNorm(h @ w_mlp2^T; ln2) + x                              transformer.py:67-71
 * q, x, out: [NB*Hq*Wq rows] with pitches q_ld / x_ld / out_ld; the query -> key-group map is that of
 * cfp_attn_apply (g = (b, y / qth, x / qtw)); no exclusion rectangle.  w_merge [D][D], w_mlp0 [2D][2D],
 * w_mlp2 [D][2D], all K-contiguous bf16.  w_q (optional, [D][D]): when given, q may be NULL and the kernel computes
 * q = x @ w_q^T (transformer.py:45) for its own rows, rounded to the storage type like a stored q.  Intermediates stay in LDS; rounding points (bf16 after the
 * apply, before each LayerNorm and after the ReLU) are those of the unfused sequence. */
int cfp_loftr_tail(const void* q, int q_ld, const float* kv, const float* ksum, const void* x, int x_ld,
                   void* out, int out_ld, const void* w_q, const void* w_merge, const void* w_mlp0, const void* w_mlp2,
                   const float* ln1_g, const float* ln1_b, const float* ln2_g, const float* ln2_b, float ln_eps,
                   int NB, int Hq, int Wq, int qth, int qtw, float v_length, float eps, int heads, int D,
                   int dtype, cfp_stream_t stream);

/* cfp_loftr_tail for a hist2image layer whose zone grid lies 1:1 over a rectangle of the token map (bf16 / f16): instead of
 * cfp_resize_bilinear (crop) -> cfp_loftr_tail -> cfp_resize_bilinear (paste) through two grid tensors, the kernel reads its x rows from
 * the map and pastes its output into it.  tok: [NB, H, W] tokens of D channels (pitch tok_ld), read and written in place; the gh x gw query
 * grid of image b is the rectangle with origin (sy, sx), which may overhang the map: grid row (b, gy, gx) is token
 * (b, sy + gy, sx + gx), reads zero outside the map (the crop's zero padding, no zone mask) and is not stored there.  The store is the
 * paste at scale 1: o = zone_valid[b][gy / p1][gx / p2] ? out : 0 (zone_valid NULL: always out), o += token when accumulate != 0, stored
 * unconditionally, rounded once.  Key groups are the zones (qth = p1, qtw = p2); w_q is required.  For finite tokens the result is
 * bit-identical to the three launches (their bilinear weights are exactly 1 and 0; what the products by 0 do to the sign of a zero
 * and to non-finite neighbours is not reproduced). */
int cfp_loftr_tail_x2i(const float* kv, const float* ksum, void* tok, int tok_ld, int H, int W, int sy, int sx,
                       const void* w_q, const void* w_merge, const void* w_mlp0, const void* w_mlp2,
                       const float* ln1_g, const float* ln1_b, const float* ln2_g, const float* ln2_b, float ln_eps,
                       int NB, int gh, int gw, int p1, int p2, const uint8_t* zone_valid, int zn, int accumulate,
                       float v_length, float eps, int heads, int D, int dtype, cfp_stream_t stream);

/* Bilinear resampling (align_corners=True) of a rectangle of an NHWC map into a rectangle of
 * another one.  The source rectangle may overhang the source map (reads 0 there: F.pad in
 * fusion.py:136).  If zone_valid != NULL, source texel (y,x) is multiplied by
 * zone_valid[b][(y/p1)*zn + x/p2] (fusion.py:144).  accumulate: 0 dst = v, 1 dst += v.
 * Only destination pixels inside the destination map are written.
 * Replaces F.interpolate in decoder.py:56 and fusion.py:141,148, the crop of fusion.py:138, the
 * zone regrouping of fusion.py:142,147,151 (which is pure addressing) and the masked
 * scatter-add of fusion.py:154-157. */
int cfp_resize_bilinear(const void* src, int src_ld, int Hs, int Ws, int sy0, int sx0, int sh, int sw,
                        void* dst, int dst_ld, int Hd, int Wd, int dy0, int dx0, int dh, int dw,
                        const uint8_t* zone_valid, int zn, int p1, int p2, int accumulate,
                        int B, int C, int dtype, cfp_stream_t stream);

/* cfp_resize_bilinear with the moving rectangle read from DEVICE memory: rec = the int32[9] zone record of cfp_zone_crop
 * (sy, sx, tzh, tzw, y0, y1, x0, x1, n_inside), so one captured graph serves every zone rectangle.
 *   rec_side 0 -- the crop of fusion.py:136-141: source rectangle (rec.sy, rec.sx, rec.tzh, rec.tzw) of the zero-extended
 *                 Hs x Ws map -> the whole Hd x Wd destination.
 *   rec_side 1 -- the paste of fusion.py:144-157: the whole Hs x Ws zone grid -> destination rectangle (rec.sy, rec.sx,
 *                 rec.tzh, rec.tzw); only its pixels inside the Hd x Wd map are written, zone_valid / accumulate as in
 *                 cfp_resize_bilinear.
 * The launch walks the whole destination map whatever the record holds; the scales (sh-1)/(dh-1) are the host's float32
 * expression evaluated on the device (bit-identical results).  tzh <= 0 or tzw <= 0: the crop writes zeros (adds nothing
 * with accumulate), the paste writes nothing.  The caller checks the record against the zone grid (tzh <= zn*p1,
 * tzw <= zn*p2) on the host: a launch cannot. */
int cfp_resize_bilinear_dev(const void* src, int src_ld, int Hs, int Ws, void* dst, int dst_ld, int Hd, int Wd,
                            const int* rec, int rec_side, const uint8_t* zone_valid, int zn, int p1, int p2,
                            int accumulate, int B, int C, int dtype, cfp_stream_t stream);

/* out[r,:] = in[r,:] + table[((r / W) % H + oy) * Wt + (r % W) + ox, :]   (table f32 [*, C])
 * Positional encodings: fusion.py:92-96 (H x W window of the [Hmax*Wmax, D] table) and
 * fusion.py:123-124 (H=1, W=Wt=16). */
int cfp_add_rowtable(const void* in, int in_ld, const float* table, void* out, int out_ld, int rows, int C,
                     int H, int W, int Wt, int oy, int ox, int dtype, cfp_stream_t stream);

/* UpSampleBN's first half in ONE launch (decoder.py:51-58): F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True) ->
 * torch.cat([up, skip], dim=1) -> conv3x3 (padding 1) + folded BatchNorm (scale / shift) + activation.  low [B,Hs,Ws,low_ld] (Cup channels),
 * skip [B,H,W,skip_ld] (Cskip channels), w [Cout][3][3][Cup + Cskip] (the concatenation's channel order), out [B,H,W,out_ld].
 * The upsampled tensor and the concatenation are never materialised: the direct 3x3 kernel computes the upsampled channel chunks into its
 * LDS halo tile (four taps blended in float32, rounded to `dtype` like a stored tensor) and fetches the skip chunks.  Bit-identical to
 * cfp_resize_bilinear + cfp_conv2d_nhwc.  bf16 / f16, Cup % 64 == 0, Cskip % 8 == 0, Cout % 8 == 0.
 * dtype = CFP_F32X3 (round 5): float32 tensors, f16x3 matrix math -- the chunk-pipelined kernel with two sources (conv3x3_halo_x3.hip); `w` is then
 * the pre-split operand of cfp_pack_w_x3 over the PADDED channel axis [Cout][9][Cup + 32 * ceil(Cskip / 32)] (zero weights on the padding);
 * Cup % 32 == 0, Cskip % 4 == 0, Cout % 4 == 0.  Equal to the pair it replaces to float32 round-off (another summation order); measured slower than
 * that pair at every decoder stage (profiles/r5_up_bench_x3.txt), so the engine takes it only under CFP_UP_FUSED_X3. */
int cfp_upsample_cat_conv3x3(const void* low, int low_ld, int Hs, int Ws, int Cup, const void* skip, int skip_ld, int Cskip,
                             const void* w, const float* scale, const float* shift, void* out, int out_ld, int B, int H, int W,
                             int Cout, int act, int dtype, cfp_stream_t stream);

/* Strided row copy out[r, 0:C] = in[r, 0:C]. */
int cfp_copy_rows(const void* in, int in_ld, void* out, int out_ld, int rows, int C, int dtype, cfp_stream_t stream);
/* Two such copies in one launch (a channel concatenation [a | b] -> out, or its backward split): copy k moves `rows` rows of Ck channels. */
int cfp_copy_rows2(const void* in0, int in0_ld, void* out0, int out0_ld, int C0, const void* in1, int in1_ld, void* out1, int out1_ld,
                   int C1, int rows, int dtype, cfp_stream_t stream);

/* rgb f32 NCHW [B,3,H,W] -> NHWC [B,H,W,8] (channels 3..7 zero) in `dtype`. */
int cfp_rgb_to_nhwc8(const float* rgb, void* out, int B, int H, int W, int dtype, cfp_stream_t stream);
/* The same for the 16-bit storage types with the input kept EXACT: channels 0-2 = rgb rounded to `dtype`, channels 3-5 = what the
 * rounding lost (rgb - hi, rounded), 6-7 = 0.  With the stem's weight rows repeating the three real channels in slots 3-5 the
 * float32 accumulators see w * (hi + lo): the float32 image the reference feeds its encoder (encoder.py:71-73), at no extra cost
 * (the stem GEMM pads every tap to 8 channel slots anyway).  bf16 / f16 only. */
int cfp_rgb_to_nhwc8_hilo(const float* rgb, void* out, int B, int H, int W, int dtype, cfp_stream_t stream);
/* f32 scalars [rows] -> [rows][8] with the value in column 0 (ToF sample depths, deltar.py:40). */
int cfp_scalar_to_rows8(const float* in, void* out, int rows, int dtype, cfp_stream_t stream);

/* ToF histogram encoder in one launch (csrc/hist_encoder.hip): HistogramEncoder.forward, encoder.py:45-50 = three HistExtractors
 * (:31-35) of three [Conv1d k=1 -> BatchNorm1d -> ReLU] layers each (PointNetEncoder, :17-24), applied to every sample point
 * independently.  hist [R] f32 (device): the R = B*Z*16 sample depths (deltar.py:40).  blob (device, f32): the parameters of the 9
 * layers; layout (HOST, 45 ints): per layer (w_off, scale_off, shift_off, cin, cout), offsets in floats into blob: W [cout][cin]
 * row-major, scale / shift [cout] = BatchNorm (+ conv bias) folded to y = relu(scale * (W x) + shift).  cin of layer 0 is 1, widths
 * are multiples of 16 up to 128.  out0 / out1 / out2: the activations after layers 3, 6, 9, [R][cout] in `dtype` (all arithmetic
 * is float32 whatever the storage type: v_mfma_f32_16x16x4_f32 on float32 activations held in LDS).  pe0 / pe1 / pe2 (device f32
 * [n_pe][cout], each may be NULL): `positional_encodings2` of the fusion block that consumes the tap, added on the way out with
 * row = sample index % n_pe (fusion.py:123-125: `feat1 + positional_encodings2`, n_pe = zone_sample_num). */
int cfp_hist_encoder(const float* hist, const float* blob, const int* layout, void* out0, void* out1, void* out2,
                     const float* pe0, const float* pe1, const float* pe2, int n_pe, int R, int dtype, cfp_stream_t stream);

/* LKPM tail in one launch (csrc/loftr_tail.hip): Block14.forward after its depthwise conv + BatchNorm + ReLU (convnext.py:48-58):
 *   out = xin + pwconv2(GELU(pwconv1(LayerNorm(t))))      LayerNorm over the D channels, eps = ln_eps (1e-6), exact-erf GELU
 * t [rows, t_ld] = the depthwise stage's output, xin [rows, x_ld] = the block's input (residual), w1 [4D][D], b1 [4D], w2 [D][4D],
 * b2 [D], ln_g / ln_b [D].  The 4D-wide hidden tensor never reaches HBM.  bf16 / f16 only; D in {32, 64, 128}. */
int cfp_lkpm_tail(const void* t, int t_ld, const void* xin, int x_ld, void* out, int out_ld, const void* w1, const float* b1,
                  const void* w2, const float* b2, const float* ln_g, const float* ln_b, float ln_eps, int rows, int D, int dtype,
                  cfp_stream_t stream);

/* Bin-width regressor + bin edges/centres, one workgroup per batch element, all f32:
 *   mean -> conv1x1 (no bias) -> Linear/LeakyReLU x2 -> Linear -> norm -> widths -> cumsum
 * Every weight matrix is passed TRANSPOSED, [n_in][n_out] (coalesced across output threads).
 * norm: 0 linear (relu + 0.1, L1-normalise), 1 softmax, 2 sigmoid (L1-normalise).
 * edges [B][nbins+1], centers [B][nbins].  Replaces decoder.py:23-36 + deltar.py:53-59. */
int cfp_bin_regressor(const float* partial, int nsplit, float inv_hw, const float* w1x1_t,
                      const float* w0_t, const float* b0, const float* w1_t, const float* b1,
                      const float* w2_t, const float* b2, float min_val, float max_val, int norm,
                      float* edges, float* centers, int B, int C, int hidden, int nbins, cfp_stream_t stream);

/* Spatial SUM of a linear 3x3 convolution's output (stride 1, zero padding 1, bias, no activation) without running the convolution:
 * from nine shifted sums of its INPUT (csrc/head.hip).  Used for DepthRegression's mean over conv1x1(unet) (decoder.py:28-29) where
 * unet = decoder.conv0(t) (decoder.py:126): the regressor branch then depends on t only and runs beside conv0.
 *   partial [B][nsplit][C] f32: channel sums of x over row splits (cfp_channel_sum); x [B,H,W,ld] (C channels, C divides 1024): the
 *   kernel reads its four border lines and corner pixels itself; w [Cout][3][3][C] float32, bias [Cout] (may be NULL) ->
 *   msum [B][Cout] = sum over all H*W output pixels (feed it to cfp_bin_regressor with nsplit = 1, inv_hw = 1/HW). */
int cfp_conv3x3_mean(const float* partial, int nsplit, const void* in, int in_ld, const float* w, const float* bias, float* msum,
                     int B, int H, int W, int C, int Cout, int dtype, cfp_stream_t stream);

/* Per-pixel softmax over nbins logits + expectation over bin centres:
 *   prob[b, n, hw] = softmax_n(logits[b*HW + hw, n]);  pred[b, hw] = sum_n prob * centers[b, n]
 * nbins is 64, 128 or 256.  prob (NCHW, `dtype`) may be NULL.  pred is f32.  Replaces nn.Softmax(dim=1) of deltar.py:19
 * and deltar.py:61. */
int cfp_bin_softmax(const void* logits, int ld, const float* centers, void* prob, float* pred,
                    int B, int HW, int nbins, int dtype, cfp_stream_t stream);

/* Per-pixel uncertainty of the bin distribution, an optional third output of the three head entry points (the `_stats` twins below:
 * the same argument lists with `float* stats` after `pred`).  With p_n the softmax over the bins (deltar.py:51), c_n the image's bin
 * centres and mu = pred = sum_n p_n c_n (deltar.py:61), stats is float32 [B][3][HW] in every dtype:
 *   plane CFP_UNC_STD      sqrt(sum_n p_n (c_n - mu)^2)   metres, >= 0 (centred two-pass form: no cancellation on a confident pixel)
 *   plane CFP_UNC_ENTROPY  -sum_n p_n ln p_n              nats, 0 .. ln nbins; from the shifted logits d_n = l_n - max as
 *                                                         ln s - (sum_n e^d_n d_n) / s with s = sum_n e^d_n: no log of a probability
 *   plane CFP_UNC_PMAX     max_n p_n = 1 / s              1 / nbins .. 1
 * computed from the float32 values the kernel holds before `prob` is rounded to its storage type.  stats == NULL is exactly the call
 * without the suffix (the same kernel instantiation); with stats given, prob and pred are bit-identical to that call. */
enum { CFP_UNC_STD = 0, CFP_UNC_ENTROPY = 1, CFP_UNC_PMAX = 2 };
int cfp_bin_softmax_stats(const void* logits, int ld, const float* centers, void* prob, float* pred, float* stats,
                          int B, int HW, int nbins, int dtype, cfp_stream_t stream);

/* The whole adaptive-bins head in one kernel (csrc/head_fused.hip):
 *   ram = conv3x3(x) (128 -> 128, decoder.py:22-27 `self.conv3x3`), logits = conv_out(ram) (1x1, 128 -> 256,
 *   deltar.py:18-19,51), prob = softmax over the 256 bins, pred = sum_n prob * centers (deltar.py:61).
 * `ram` and the logits never reach HBM.  x [B*H*W, x_ld] NHWC 16-bit with 128 channels; w3 [128][3*3*128] as cfp_conv2d_nhwc
 * lays weights out; scale3 / shift3 [128] f32 (may be NULL = 1 / 0; depth_head.conv3x3 has a bias and no activation);
 * wout_perm [256][128] with the input-channel axis permuted for the kernel's fragment order: position 32 kb + 8 q + e holds
 * channel 32 kb + 16 (e >> 2) + 4 q + (e & 3) (kb, q in 0..3, e in 0..7); with CFP_HEAD_WOUT_HILO a second [256][128] plane
 * follows holding round16(W - hi) so conv_out's weights act with ~22 significant bits; CFP_HEAD_RAM_HILO feeds ram to the
 * second GEMM as hi + lo (no 16-bit rounding of ram).  bias_out [256], centers [B,256] f32; prob [B,256,H*W] (NCHW, `dtype`,
 * may be NULL); pred [B*H*W] f32; ram_out [B*H*W,128] (`dtype`, may be NULL: test hook).  bf16 / f16 only; H*W % 16 == 0 and H*W >= 128. */
enum { CFP_HEAD_WOUT_HILO = 1, CFP_HEAD_RAM_HILO = 2 };
int cfp_depth_head_fused(const void* x, int x_ld, const void* w3, const float* scale3, const float* shift3,
                         const void* wout_perm, const float* bias_out, const float* centers, void* prob, float* pred,
                         void* ram_out, int B, int H, int W, int flags, int dtype, cfp_stream_t stream);
/* The same with the uncertainty planes (see cfp_bin_softmax_stats): stats [B][3][H*W] f32, may be NULL. */
int cfp_depth_head_fused_stats(const void* x, int x_ld, const void* w3, const float* scale3, const float* shift3,
                               const void* wout_perm, const float* bias_out, const float* centers, void* prob, float* pred,
                               float* stats, void* ram_out, int B, int H, int W, int flags, int dtype, cfp_stream_t stream);

/* decoder.conv0 + the whole head in one kernel (csrc/head_conv0.hip): unet = conv0(t) (3x3, 32 -> 128, bias, no activation;
 * decoder.py conv0) feeds cfp_depth_head_fused's chain (decoder.py:22-27, deltar.py:51-61) without reaching HBM.  A workgroup computes the
 * 18 x 18 halo of `unet` of its 16 x 16 pixel tile from t, rounded to `dtype` exactly as cfp_conv2d_nhwc stores it and zero outside the
 * image, so prob and pred are those of the two launches bit for bit.  t [B*H*W, t_ld] NHWC 16-bit with 32 channels; w0 [128][3*3*32],
 * scale0 / shift0 [128] f32 (may be NULL = 1 / 0); the other operands as cfp_depth_head_fused takes them (one Wout plane: no hi + lo
 * options, no uncertainty planes, no ram_out).  flags: 0.  bf16 / f16 only; H % 16 == 0 and W % 16 == 0, otherwise CFP_ESHAPE (run the
 * pair); CFP_ESHAPE too if the device does not grant the kernel's 162 944 bytes of LDS. */
int cfp_depth_head_conv0_fused(const void* t, int t_ld, const void* w0, const float* scale0, const float* shift0, const void* w3,
                               const float* scale3, const float* shift3, const void* wout_perm, const float* bias_out,
                               const float* centers, void* prob, float* pred, int B, int H, int W, int flags, int dtype,
                               cfp_stream_t stream);

/* Fused bin head: logits = x @ w^T + bias never leave the chip:
 *   1x1 conv (Cin -> 256) on the matrix cores, row softmax, expectation, optional prob write.
 * Replaces conv_out (deltar.py:18-19,51) + deltar.py:61.  nbins == 256.  dtype CFP_BF16 / CFP_F16: 16-bit x, w [256][Cin] and prob;
 * dtype CFP_F32X3 (the default numerics of the drop-in boundary): float32 x, `w` = cfp_pack_w_x3 of the [256][Cin] weights, float32 prob
 * -- the reference's own output type -- written by the kernel; HW % 4 == 0. */
int cfp_bin_head_fused(const void* x, int x_ld, const void* w, const float* bias, const float* centers,
                       void* prob, float* pred, int B, int HW, int Cin, int dtype, cfp_stream_t stream);
/* The same with the uncertainty planes (see cfp_bin_softmax_stats): stats [B][3][HW] f32, may be NULL. */
int cfp_bin_head_fused_stats(const void* x, int x_ld, const void* w, const float* bias, const float* centers,
                             void* prob, float* pred, float* stats, int B, int HW, int Cin, int dtype, cfp_stream_t stream);

/* ---- training step pieces -------------------------------------------------- */

/* SILogLoss.forward (loss.py:9-19), f32: pred [B,1,Hp,Wp] is bilinearly resized (align_corners=True) to the
 * target size when `interpolate`, g = log p - log t over the pixels with mask != 0 (mask may be NULL = all),
 * loss = 10 * sqrt(var_unbiased(g) + 0.15 * mean(g)^2).  stats[4] (device, f32) = {loss, mean(g), n, Dg}.
 * ws (cfp_silog_ws_bytes) keeps g and 1/p for the backward pass.  Reductions are f64 partial sums combined
 * in a fixed order (deterministic). */
size_t cfp_silog_ws_bytes(int B, int Ht, int Wt);
int cfp_silog_loss_fwd(const float* pred, int Hp, int Wp, const float* target, const unsigned char* mask, int Ht, int Wt,
                       int B, int interpolate, void* ws, size_t ws_bytes, float* stats, cfp_stream_t stream);
/* d loss / d pred (same ws / stats as the forward call), scaled by grad_loss; a gather, no atomics. */
int cfp_silog_loss_bwd(const void* ws, const float* stats, float grad_loss, int Hp, int Wp, int Ht, int Wt, int B,
                       int interpolate, float* grad_pred, cfp_stream_t stream);

/* Bin-centre chamfer loss (the `w_chamfer` term of the AdaBins training recipe; none in the reference), value and gradient, f32.
 * Per image b:  centres c_p = 0.5 (e_p + e_{p+1}), p = 0..P-1, from edges [B,P+1] (strictly increasing: the caller's duty, not checked);
 * target points T_b = { target[b,y,x] : mask[b,y,x] != 0 } at the full target size (mask NULL: target >= 1e-3), N_b = |T_b|;
 *   L_b = (1/P) sum_p min_{t in T_b} (c_p - t)^2 + (1/N_b) sum_{t in T_b} min_p (c_p - t)^2,      L = (1/B) sum_b L_b.
 * An image with N_b = 0 contributes 0 to the loss and 0 to the gradient; the denominator stays B.  Ties: the lower centre index wins,
 * and the lower target value wins.  loss [1+B] (device) = {L, L_0 .. L_{B-1}}; grad_centers [B,P] (may be NULL) = grad_scale * dL/dc,
 * which cfp_bin_centers_bwd carries on to the widths.  One pass over the pixels (a binary search over the sorted centres per pixel, no
 * N x P comparison), a finalising launch per image and a one-wave mean.  Deterministic like cfp_silog_loss_fwd: per-workgroup partials
 * in ws (cfp_bins_chamfer_ws_bytes, 16-byte aligned) combined in index order, f64 sums in fixed-order trees, and the only atomics are
 * integer ones in LDS (order-independent): min / max of the targets per interval, and the per-centre sum of d = t - c_nearest in fixed
 * point with quantum 2^-40, |d| clamped to 2047 (depths are metres), moved to f64 every 4096 pixels of a workgroup, so no image size
 * overflows it.  No host sync, no allocation, graph-capturable.  1 <= P <= 1024 and B*Ht*Wt < 2^31, otherwise CFP_ESHAPE. */
size_t cfp_bins_chamfer_ws_bytes(int B, int Ht, int Wt, int P);
int cfp_bins_chamfer(const float* edges, const float* target, const unsigned char* mask, int B, int Ht, int Wt, int P,
                     float grad_scale, void* ws, size_t ws_bytes, float* loss, float* grad_centers, cfp_stream_t stream);

/* torch.optim.AdamW step (train.py:82,131) over one contiguous segment of flat f32 buffers: `step` is the
 * 1-based step count of the group, beta1 may change per step (OneCycleLR cycles it, train.py:90-94).
 * grad_scale (device, may be NULL) multiplies the gradient first: the clip factor of cfp_grad_clip_factor. */
int cfp_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                   cfp_stream_t stream);
/* nn.utils.clip_grad_norm_ (train.py:130) without a host sync: out[0] = min(1, max_norm / (||grad||_2 + 1e-6)),
 * out[1] = ||grad||_2, both on the device; `out` holds 3 floats.  OVERFLOW GUARD of the 16-bit training modes: when the norm is not
 * finite (an inf / nan anywhere in the gradient) out[0] = -1 and out[2] is incremented; cfp_adamw_step given such a grad_scale leaves
 * parameters and moments untouched (the step is skipped, like torch.cuda.amp.GradScaler does).  `grad` must be 16-byte aligned. */
size_t cfp_grad_clip_ws_bytes(void);
int cfp_grad_clip_factor(const float* grad, long long n, float max_norm, void* ws, size_t ws_bytes, float* out,
                         cfp_stream_t stream);

/* ---- data path either side of the model ------------------------------------------------- */

/* ToF zone-histogram simulation from ground-truth depth, a whole batch per launch.  Replaces the per-sample CPU
 * functions get_hist_parallel (src/utils/dataloader.py:83-134) and the uniform branch of
 * sample_point_from_hist_parallel (:65-80) that the data-loader workers call (src/dataloader/nyu.py:154,179).
 *   depth    [B] images of H x W f32, `img_stride` elements apart (device)
 *   zone grid: zone_num x zone_num squares of zone_px pixels whose top-left zone starts at (sy0 + off, sx0 + off);
 *            the reference uses sy0 = int((H - zone_px*zone_num)/2), 64 px zones when training and 56 px otherwise
 *            (:94-103).  offsets (device, [B] int32, may be NULL) is the per-sample `train_zone_random_offset`
 *            draw (:98-100), clamped to +-offset_bound; the grid must stay inside the image for that bound.
 *   histogram: torch.histc(bins, min=0, max=max_distance) in f32 (:104), bin 0 cleared and floor_count (20)
 *            subtracted (:108-109), strongest run of consecutive non-zero bins kept (:110-116), moments over bin
 *            centres built from multiples of bin_width (0.04) in f64 (:118,127-130).
 *   w0, w1   [nsamp] f32 (device): torch.linspace(1,0,nsamp) / torch.linspace(0,1,nsamp) as the HOST evaluates
 *            them (tensor_linspace, :42-57; ATen's vectorised linspace differs in the last bit between hosts);
 *            with sample_mode CFP_TOF_SAMPLE_ICDF w0 is the erfinv table of cfp_tof_sample_points and w1 may be NULL.
 * Outputs (device): fh [B,Z,2] f64 (mu, sigma); rect [B,Z,4] f32 (sy,sx,ey,ex); mask [B,Z] u8; pts [B,Z,nsamp] f32
 * (zero where mask is 0); hist_out [B,Z,bins] i32 (may be NULL): the counts that survive cluster selection. */
int cfp_tof_hist_sim(const float* depth, long long img_stride, int B, int H, int W, int zone_num, int zone_px, int sy0,
                     int sx0, const int* offsets, int offset_bound, float max_distance, int bins, double bin_width,
                     int floor_count, const float* w0, const float* w1, int nsamp, int sample_mode, double* fh, float* rect,
                     unsigned char* mask, float* pts, int* hist_out, cfp_stream_t stream);
/* The sampling step alone (sample_point_from_hist_parallel, dataloader.py:65-80), for callers that keep the reference's
 * two calls.  sample_mode CFP_TOF_SAMPLE_UNIFORM (--sample_uniform, :74-79): pts[z, t] = f32(w0[t]*(mu-3 sigma) +
 * w1[t]*(mu+3 sigma)) in f64.  CFP_TOF_SAMPLE_ICDF (the argparse default, :69-73): Normal(mu, sigma).icdf at the
 * nsamp ppf points arange(1e-3, 1, 0.998/(nsamp-1)): pts[z, t] = f32(mu + (sigma * w0[t]) * sqrt(2)) in f64 with
 * w0[t] = erfinv(2 ppf_t - 1) evaluated in FLOAT32 on the host, as torch does (the ppf tensor is f32); w1 is unused
 * and may be NULL.  pts is 0 where !mask[z]. */
int cfp_tof_sample_points(const double* fh, const unsigned char* mask, const float* w0, const float* w1, long long nzones,
                          int nsamp, int sample_mode, float* pts, cfp_stream_t stream);
/* ToF degradation between cfp_tof_hist_sim and the model: random zone dropout (src/dataloader/nyu.py:155-158) and Gaussian range
 * noise (what nyu.py:159-163 intended; the reference adds it to a copy), then the samples of the result.  One launch per batch, one
 * workgroup per image, nothing returns to the host.
 *   fh [B,Z,2] f64 (mu, sigma) and mask [B,Z] u8 as cfp_tof_hist_sim writes them; w0, w1, nsamp, sample_mode as
 *   cfp_tof_sample_points takes them.  All pointers are device pointers.
 *   Random numbers  Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (i, b, step, stream): b the image, stream 0
 *            the dropout with i the draw index, stream 1 the noise with i the zone index.  An image's result depends on (seed, step,
 *            b) and its own inputs only, not on B or on the launch geometry.
 *   Dropout  V = the valid zones of image b in ascending order, n = |V|, k = (int)(n * drop) with the product in f64.  For j < k
 *            zone V[(word0(j) * n) >> 32] (64-bit product, word0 the first word of counter (j, b, step, 0)) loses its validity:
 *            draws with replacement, as rng.choice(idx, k) of the reference, so duplicates are expected and at most k zones are
 *            dropped.  The multiply-shift has a bias below n / 2^32.
 *   Noise    after the dropout, on the zones that are still valid: with the words w of counter (z, b, step, 1) zone z is hit when
 *            w0 * 2^-32 < noise_prob, and then mu += noise_mean + noise_sigma * sqrt(-2 ln((w1 + 1) * 2^-32)) * cos(2 pi * w2 * 2^-32)
 *            (Box-Muller) in f64.  sigma is untouched and mu is not clamped.
 *   Samples  pts[b, z, :] as cfp_tof_sample_points gives them for the resulting (mu, sigma); a zone that is not valid in mask_out
 *            gets an all-zero row (dropout first, then sampling: nyu.py:155-158 before :179).
 * Outputs: mask_out [B,Z] u8; fh_out [B,Z,2] f64 (may be NULL when noise_prob == 0); pts [B,Z,nsamp] f32; counts [B,3] i32 (may be
 * NULL) = {valid before, distinct zones dropped, zones that received noise}.  With drop = 0 and noise_prob = 0 the outputs equal
 * mask, fh and cfp_tof_sample_points(fh, mask) bit for bit.
 * Limits: 1 <= Z <= 256 (16 x 16 is the largest grid in use), B * Z < 2^31, 0 <= drop <= 1, 0 <= noise_prob <= 1, noise_sigma >= 0;
 * anything else is CFP_EINVAL / CFP_ESHAPE before any launch. */
int cfp_tof_degrade(const double* fh, const unsigned char* mask, int B, int Z, double drop, double noise_prob, double noise_mean,
                    double noise_sigma, unsigned long long seed, unsigned int step, const float* w0, const float* w1, int nsamp,
                    int sample_mode, unsigned char* mask_out, double* fh_out, float* pts, int* counts, cfp_stream_t stream);

/* Depth-evaluation metrics per image without leaving the device: compute_errors (src/utils/metrics.py:4-24 =
 * evaluate_all.py:15-35) fused with the protocol around it.
 *   mode 0 = evaluate_all.py:38-41,80-84: pred clipped to [lo, hi] at model resolution, then bilinear
 *            (align_corners=True) to H x W; valid pixels lo < gt < hi (args.min_depth / args.max_depth).
 *   mode 1 = train.py:187-199 (validate): bilinear first, then clamp to [lo, hi], nan -> lo; valid pixels
 *            lo < gt < hi (args.min_depth_eval / args.max_depth_eval).
 *   pred [B,Hp,Wp] f32, gt [B,H,W] f32 (device); interpolate = 0 requires equal sizes.
 * out [B,10] f64 (device) = {a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel, n_valid}; an image with
 * n_valid = 0 yields NaN metrics (the reference skips it).  Per-pixel terms f32, sums f64 in a fixed order. */
size_t cfp_eval_metrics_ws_bytes(int B);
int cfp_eval_metrics(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, int mode,
                     float lo, float hi, void* ws, size_t ws_bytes, double* out, cfp_stream_t stream);

/* Sparsification curves, AUSE and AURG of the uncertainty planes (CFP_UNC_*) per image without leaving the device.
 *   Inputs  pred [B,Hp,Wp] f32, unc [B,3,Hp,Wp] f32 (planes CFP_UNC_STD / ENTROPY / PMAX), gt [B,H,W] f32, bounds lo < hi,
 *           mode 0 or 1 exactly as cfp_eval_metrics (clip / bilinear order, nan -> lo in mode 1, valid pixels lo < gt < hi),
 *           steps = K with 1 <= K <= 100.
 *   Protocol  the prediction v at a valid pixel is what cfp_eval_metrics evaluates there; each uncertainty plane is brought to
 *           H x W with the same align-corners bilinear taps, without a clip (interpolate = 0: read directly, equal sizes required).
 *   Terms   float32: d = g - v, t0 = d*d, t1 = fabsf(d)/g.
 *   Scores  float32, a larger score is removed first: s0 = std, s1 = entropy, s2 = 1 - pmax, s3 = t0 (the RMSE oracle),
 *           s4 = t1 (the abs-rel oracle); rankings are numbered CFP_SPARS_*.  Float ordering with -0 == +0 and NaN above +inf
 *           (all NaNs tie).
 *   Curves  for ranking r, point k = 0..K-1 and N valid pixels the kept count is n_k = N - floor(k*N/K) (integers, n_k >= 1 when
 *           N >= 1) and the kept set is the n_k pixels with the smallest s_r.  A group of exactly equal scores that straddles the
 *           boundary with t of its c members kept contributes t/c of the group's sums, so no value depends on a tie-break or on
 *           pixel order.  With S_m the float64 sum of t_m over the kept set:
 *             curves[b][r][0][k] = sqrt(S_0 / n_k)  (RMSE)      curves[b][r][1][k] = S_1 / n_k  (abs-rel)
 *   Summary for the uncertainty rankings u = 0..2 and metric m, with e0 = curve[.][m][0] (the same for every ranking) and
 *           o = 3 + m:  AUSE = summary[b][u][m][0] = mean_k (curve[u][m][k] - curve[o][m][k]) / e0
 *                       AURG = summary[b][u][m][1] = mean_k (e0 - curve[u][m][k]) / e0
 *   n_valid[b] = N.  If N == 0 or e0 == 0 every curve and summary value of that image is NaN.
 * The ranking is exact on the full float32 score (radix select, no quantised keys); the sums are exact integer accumulations
 * rounded to float64 once, so two calls on the same tensors give identical bits.  No host synchronisation, no global atomics;
 * everything runs on `stream` in the caller's workspace (cfp_unc_sparsification_ws_bytes bytes, 8-byte aligned). */
enum { CFP_SPARS_STD = 0, CFP_SPARS_ENTROPY, CFP_SPARS_PMAX, CFP_SPARS_ORACLE_RMSE, CFP_SPARS_ORACLE_ABSREL };
size_t cfp_unc_sparsification_ws_bytes(int B, int H, int W, int steps);
int cfp_unc_sparsification(const float* pred, const float* unc, int Hp, int Wp, const float* gt, int H, int W, int B,
                           int interpolate, int mode, float lo, float hi, int steps, void* ws, size_t ws_bytes,
                           double* curves /* [B][5][2][steps] */, double* summary /* [B][3][2][2]: AUSE, AURG */,
                           double* n_valid /* [B] */, cfp_stream_t stream);

/* The metrics of cfp_eval_metrics split by region and by depth range, per image, in one pass, without leaving the device.
 *   Inputs  pred, gt, interpolate, mode, lo < hi exactly as cfp_eval_metrics: the float32 prediction evaluated at a pixel and the
 *           validity rule lo < gt < hi are the same, bit for bit.  rect [B,Z,4] f32 (sy, sx, ey, ex) and mask [B,Z] u8 on the
 *           device, read per image (the model's rect_data / mask inputs).
 *   Regions the FoV rectangle is the reference's `my_mask` (src/dataloader/nyu.py:182-187): aa = max(0, trunc(rect[b][0][0])),
 *           bb = max(0, trunc(rect[b][0][1])), cc = min(H, trunc(rect[b][Z-1][2])), dd = min(W, trunc(rect[b][Z-1][3])); pixel
 *           (y, x) is inside iff aa <= y < cc && bb <= x < dd (empty if cc <= aa or dd <= bb; no negative-slice wrap-around).
 *             CFP_REGION_ALL           every valid pixel
 *             CFP_REGION_FOV_IN        inside the FoV rectangle            CFP_REGION_FOV_OUT  not inside it
 *             CFP_REGION_ZONE_VALID    inside the FoV rectangle and inside the rectangle of some zone z with mask[b][z] != 0
 *                                      (sy <= y < ey && sx <= x < ex, compared in float)
 *             CFP_REGION_ZONE_INVALID  inside the FoV rectangle and not ZONE_VALID (a dropped zone, or a gap between zones)
 *   Ranges  n_edges = E, 0 <= E <= 7; `edges` is a HOST array of E finite, strictly increasing floats -- the one host pointer of the
 *           call, copied into the kernel arguments (may be NULL when E == 0).  A pixel's range index is the number of edges e with
 *           gt >= e in float32: E + 1 ranges.
 *   out [B][5][Q][10] f64 (device), Q = 1 if E == 0 else E + 2: region CFP_REGION_*, then q = 0 "all depths" and q = 1 + r range r,
 *           then the ten values of cfp_eval_metrics (nine metrics, pixel count).  A segment without a valid pixel has NaN metrics
 *           and count 0.
 * Every valid pixel is accumulated into exactly one cell (zone class x range); every entry of `out` is finalised from sums of cell
 * sums.  Per-pixel terms f32, sums f64, no floating-point atomics, fixed summation order: two calls on the same tensors give identical
 * bits.  No host synchronisation; workspace of cfp_eval_metrics_regions_ws_bytes(B) bytes, 8-byte aligned. */
enum { CFP_REGION_ALL = 0, CFP_REGION_FOV_IN, CFP_REGION_FOV_OUT, CFP_REGION_ZONE_VALID, CFP_REGION_ZONE_INVALID };
size_t cfp_eval_metrics_regions_ws_bytes(int B);
int cfp_eval_metrics_regions(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, int mode,
                             float lo, float hi, const float* rect /* [B][Z][4] */, const unsigned char* mask /* [B][Z] */, int Z,
                             const float* edges /* host, [n_edges] */, int n_edges, void* ws, size_t ws_bytes,
                             double* out /* [B][5][Q][10] */, cfp_stream_t stream);

/* Back-projection of the prediction to 3-D points in the camera frame, with surface normals, without leaving the device: the step
 * after the depth map for whoever consumes ToF depth completion (robotics, AR, reconstruction).
 *   Inputs  pred [B,Hp,Wp] f32 (device); H, W, interpolate, lo < hi as cfp_eval_metrics in mode 0; K [B][4] f32 ON THE DEVICE: the
 *           pinhole intrinsics (fx, fy, cx, cy) in pixels of the H x W grid, per image -- the numbers the reference's ZJU-L5 loader
 *           carries as K_list and never uses (src/dataloader/zjuL5.py:66-71).  fx and fy cannot be checked without a
 *           synchronisation: the caller guarantees that all four are finite and that fx, fy are not 0.
 *   Depth   d(x, y) is the float32 value cfp_eval_metrics evaluates at that pixel in mode 0 (evaluate_all.py:40-41): clip to [lo, hi] at
 *           model resolution, then the align-corners bilinear blend, a dimension of unchanged size read twice with weights (1, 0); with
 *           interpolate = 0 the sizes must be equal and d is the clipped value.  One implementation (csrc/metrics_pred.h): bit for bit.
 *   Point   float32, in this order of operations (no fused multiply-add):
 *             rx = ((float)x - cx) / fx     ry = ((float)y - cy) / fy     P(x, y) = (rx * d, ry * d, d)
 *           Plain arithmetic: a NaN depth gives a NaN point.
 *   Normal  from the clamped neighbours x0 = max(x - 1, 0), x1 = min(x + 1, W - 1), k = x1 - x0, xm = 0.5f * (x0 + x1), with
 *           d0 = d(x0, y), d1 = d(x1, y), in a form without the cancellation of a point difference:
 *             T_x = (d1 - d0) * r_m + (d1 + d0) * (0.5f * k / fx) * e_1      r_m = ((xm - cx) / fx, ry, 1),  e_1 = (1, 0, 0)
 *           and T_y likewise in y (y0, y1, ym, second unit vector, r_m = (rx, (ym - cy) / fy, 1)).  In exact arithmetic
 *           T_x = P(x1, y) - P(x0, y).  n = normalize(T_y x T_x): for fx, fy > 0 it faces the camera (n . P < 0), a fronto-parallel
 *           wall gives (0, 0, -1).  If one of the five depths involved (the pixel's own and its four neighbours') is not finite, or the
 *           length of the cross product is 0 or not finite, the normal is (0, 0, 0); so every normal is 0 when H == 1 or W == 1.
 *   Outputs points [B,H,W,3] f32; normals [B,H,W,3] f32 or NULL (not computed).
 * One launch, no host synchronisation, no allocation, no workspace. */
int cfp_depth_unproject(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                        const float* K /* device, [B][4]: fx fy cx cy */, float* points /* [B][H][W][3] */,
                        float* normals /* [B][H][W][3] or NULL */, cfp_stream_t stream);

/* Order-preserving selection of the points of such a map (stream compaction) by grid stride, range and uncertainty, per image, without
 * a host synchronisation.
 *   Inputs  points [B,H,W,3] f32, normals [B,H,W,3] f32 or NULL; stride >= 1; z_near < z_far; an optional uncertainty plane: unc
 *           (NULL: none) points to image 0's plane of Hu x Wu f32, image b's lies unc_stride ELEMENTS further per image (a plane of the
 *           model's [B,3,h,w] uncertainty tensor: stride 3 * h * w), with the closed interval unc_lo <= unc_hi.  When Hu x Wu differs
 *           from H x W the plane is brought to the H x W grid with the align-corners bilinear taps of the prediction, without a clip
 *           (as cfp_unc_sparsification does); otherwise it is read directly.
 *   Kept    pixel (x, y) of image b iff  x % stride == 0 && y % stride == 0,  Z = points[b][y][x][2] is finite and
 *           z_near < Z < z_far,  and -- with a plane -- unc_lo <= u(x, y) <= unc_hi (a NaN u fails).
 *   Outputs the kept pixels of image b in row-major pixel order (a stable compaction) in rows 0 .. min(count, cap) - 1 of
 *           out_points [B,cap,3] f32, out_normals [B,cap,3] f32 (given exactly when normals is) and out_index [B,cap] i32 = y * W + x.
 *           counts [B] i32 is the TRUE number kept, also when it exceeds cap (the caller detects the overflow when it reads the counts
 *           anyway).  Rows at or beyond min(count, cap) are not touched.
 * Three launches -- per-chunk counts, one exclusive scan per image, scatter -- and no atomics: two calls on the same tensors give
 * identical bits.  Workspace of cfp_points_compact_ws_bytes(B, H, W, stride) bytes, 8-byte aligned; 0 for arguments that make no sense. */
size_t cfp_points_compact_ws_bytes(int B, int H, int W, int stride);
int cfp_points_compact(const float* points, const float* normals, int H, int W, int B, int stride, float z_near, float z_far,
                       const float* unc, int Hu, int Wu, long long unc_stride, float unc_lo, float unc_hi, int cap,
                       float* out_points /* [B][cap][3] */, float* out_normals /* [B][cap][3] or NULL */,
                       int* out_index /* [B][cap] */, int* counts /* [B] */, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Forward warp of the prediction into another view, with a z-buffer, without leaving the device: the previous frame's depth carried into
 * the current camera (temporal fusion), or the completed depth seen from the ToF sensor or a second camera (RGB-D registration).
 *   Inputs  pred [B,Hp,Wp] f32; H, W, interpolate, lo < hi as cfp_depth_unproject (a full-resolution state goes in with Hp == H,
 *           interpolate = 0 and infinite bounds); K_src, K_dst [B][4] f32 ON THE DEVICE: (fx, fy, cx, cy) of the H x W source grid and of
 *           the Hd x Wd target grid, under the caller contract of cfp_depth_unproject; T [B][12] f32 ON THE DEVICE: row-major [R|t],
 *           P' = R P + t in the camera frame of cfp_depth_unproject (x right, y down, z forward); splat 1 or 2; z_near > 0.
 *   Source  d = d(x, y) of cfp_depth_unproject (csrc/metrics_pred.h, bit for bit).  A source whose d is not finite, or d <= 0, is skipped.
 *   Point   float32, in this order of operations (no fused multiply-add):
 *             X = ((float)x - cx) / fx * d     Y = ((float)y - cy) / fy * d     Z = d
 *             X' = (T[0] * X + T[1] * Y) + T[2] * Z + T[3]      Y' likewise with T[4..7], Z' with T[8..11]   (left to right)
 *           A point is skipped unless Z' is finite and Z' >= z_near.  Then  u = fx' * (X' / Z') + cx',  v = fy' * (Y' / Z') + cy'.
 *   Splat   splat = 1 hits the pixel (floorf(u + 0.5f), floorf(v + 0.5f)); splat = 2 hits the four pixels floorf(u) + {0, 1},
 *           floorf(v) + {0, 1}, which closes the cracks of a mild magnification.  A hit outside 0 <= column < Wd, 0 <= row < Hd is dropped;
 *           the test is made on the float values, before any conversion to int (a NaN or huge u, v hits nothing).
 *   Z-buffer  one 64-bit unsigned atomic minimum per hit on ws[b][row][column], with the key (bits(Z') << 32) | (y * W + x): positive
 *           floats order like their bits, so the nearest surface wins and a tie in depth goes to the lowest source index.  An integer
 *           minimum does not depend on the order of arrival: two calls on the same tensors give identical bits.
 *   Outputs depth_out [B,Hd,Wd] f32 = Z' of the winning key, index_out [B,Hd,Wd] i32 = its source y * W + x; a pixel nothing hit gets NaN
 *           and -1.  plane_out [B,Hd,Wd] f32 (given exactly when plane is): a map that travels with the depth (a variance or std map) --
 *           plane points to image 0's Hu x Wu f32, image b's lies plane_stride ELEMENTS further, brought to the H x W grid like the
 *           uncertainty plane of cfp_points_compact -- read at the winning source pixel; NaN where nothing hit.
 * Three launches (fill the workspace with all ones, splat, resolve) on `stream`, no host synchronisation, no allocation.  Workspace of
 * cfp_depth_reproject_ws_bytes(B, Hd, Wd) = 8 bytes per target pixel, 8-byte aligned; 0 for a non-positive argument. */
size_t cfp_depth_reproject_ws_bytes(int B, int Hd, int Wd);
int cfp_depth_reproject(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                        const float* K_src /* device, [B][4] */, const float* T /* device, [B][12] */,
                        const float* K_dst /* device, [B][4] */, int Hd, int Wd, int splat, float z_near,
                        const float* plane /* or NULL */, int Hu, int Wu, long long plane_stride, float* depth_out /* [B][Hd][Wd] */,
                        int* index_out /* [B][Hd][Wd] */, float* plane_out /* [B][Hd][Wd] or NULL */, void* ws, size_t ws_bytes,
                        cfp_stream_t stream);

/* Fusion of the current prediction with a prior on the same grid (the previous state warped by cfp_depth_reproject) by their variances,
 * per pixel, with a gate that keeps a changed scene or an uncovered surface from being averaged away.
 *   Inputs  cur [B,Hp,Wp] f32; H, W, interpolate, lo < hi as cfp_depth_unproject; cur_std: image 0's Hu x Wu f32 plane, image b's
 *           std_stride ELEMENTS further, brought to H x W like the plane of cfp_depth_reproject; std_floor > 0; prior_depth, prior_var
 *           [B,H,W] f32; process_var >= 0 (what the prior's variance grows by per step); gate_k >= 0, gate_abs >= 0.
 *   Pixel   float32, in this order:  c = d(x, y);  s = the std plane at the pixel, sf = s > std_floor ? s : std_floor (a NaN s gives
 *           the floor), vc = sf * sf;  p = prior_depth, vp0 = prior_var: the prior is PRESENT iff both are finite;  vp = vp0 + process_var.
 *             c finite, prior absent                                    -> (c, vc)
 *             c not finite, prior present                               -> (p, vp)                                      counted FILLED
 *             c not finite, prior absent                                -> (NaN, +inf)
 *             both, |p - c| > gate_k * sqrtf(vc + vp) + gate_abs        -> (c, vc)                                      counted REJECTED
 *             both, inside the gate:  w = vc / (vc + vp)                -> (c + w * (p - c), (vc * vp) / (vc + vp))     counted FUSED
 *   Outputs out_depth, out_var [B,H,W] f32 (they may be prior_depth, prior_var themselves: a pixel is read before it is written); counts [B][4] i32 = {prior present, fused, rejected, filled};
 *           stats [B][2] f64 = {sum |p - c|, sum (p - c)^2} over the pixels where both are present, before the gate: float32 terms
 *           ((p - c) * (p - c) rounded once), float64 sums -- the temporal consistency of two consecutive frames.
 * Two launches: per-workgroup partial sums into the workspace, then one workgroup per image finishes them in a fixed order; no
 * floating-point atomics: two calls on the same tensors give identical bits.  No host synchronisation, no allocation.  Workspace of
 * cfp_depth_fuse_ws_bytes(B, H, W) bytes, 8-byte aligned; 0 for a non-positive argument. */
enum { CFP_FUSE_PRIOR = 0, CFP_FUSE_FUSED, CFP_FUSE_REJECTED, CFP_FUSE_FILLED };
size_t cfp_depth_fuse_ws_bytes(int B, int H, int W);
int cfp_depth_fuse(const float* cur, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi, const float* cur_std,
                   int Hu, int Wu, long long std_stride, float std_floor, const float* prior_depth /* [B][H][W] */,
                   const float* prior_var /* [B][H][W] */, float process_var, float gate_k, float gate_abs,
                   float* out_depth /* [B][H][W] */, float* out_var /* [B][H][W] */, int* counts /* [B][4] */,
                   double* stats /* [B][2] */, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* A world-anchored map: a truncated signed distance field (TSDF) whose per-voxel weight is the inverse-variance sum cfp_depth_fuse keeps
 * per pixel.  cfp_tsdf_integrate fuses one frame into the volume, cfp_tsdf_raycast turns the volume back into depth, normals and std in
 * any view.  Common to both:
 *   Volume  float [B,Dz,Dy,Dx,2] ON THE DEVICE, 8-byte aligned: (F, Wt) per voxel, x fastest; voxel (i, j, k) has its centre at
 *           origin + voxel * (i, j, k) in the world frame; ox, oy, oz (finite) and voxel > 0 are host floats.  Empty: F = 1, Wt = 0.
 *   Camera  K [B][4] f32 ON THE DEVICE (fx, fy, cx, cy) under the caller contract of cfp_depth_unproject; T [B][12] f32 ON THE DEVICE:
 *           row-major [R|t], camera-from-world, Pc = R Pw + t in the camera frame of cfp_depth_unproject (x right, y down, z forward).
 * Float32 in the order written here, no fused multiply-add.
 *
 * cfp_tsdf_integrate
 *   Inputs  pred [B,Hp,Wp] f32; H, W, interpolate, lo < hi as cfp_depth_unproject; std (NULL: every observation weighs 1): image 0's
 *           Hu x Wu f32 plane, image b's std_stride ELEMENTS further, brought to H x W like the plane of cfp_depth_reproject;
 *           std_floor, trunc, z_near, w_max positive and finite.
 *   Voxel   Xw = ox + voxel * (float)i     Yw = oy + voxel * (float)j     Zw = oz + voxel * (float)k
 *           Xc = (T[0] * Xw + T[1] * Yw) + T[2] * Zw + T[3]      Yc likewise with T[4..7], Zc with T[8..11]   (left to right)
 *           Skipped unless Zc is finite and Zc >= z_near.  Then  u = fx * (Xc / Zc) + cx,  v = fy * (Yc / Zc) + cy  and the pixel is
 *           (floorf(u + 0.5f), floorf(v + 0.5f)), tested against 0 <= column < W, 0 <= row < H on the float values, before any
 *           conversion to int (a NaN or huge u, v reads nothing).  d = d(column, row) of cfp_depth_unproject (csrc/metrics_pred.h, bit
 *           for bit); skipped unless d is finite and d > 0 -- otherwise the voxel has SEEN a valid depth.
 *             sdf = d - Zc;  sdf < -trunc: the voxel lies BEHIND the surface, skipped;  f = fminf(1, sdf / trunc)
 *             s = the std plane at the pixel, sf = s > std_floor ? s : std_floor (a NaN s gives the floor), w = 1 / (sf * sf);
 *             without a plane w = 1.  An observation whose w is 0 or not finite (an infinite std) is skipped.
 *             F' = (F * Wt + f * w) / (Wt + w)     Wt' = fminf(Wt + w, w_max)                                          UPDATED
 *           A skipped voxel is neither read nor written.
 *   Outputs the volume in place; counts [B][3] i32 = {valid depth seen, updated, behind the surface}, overwritten.
 * One thread per voxel, x along the lanes.  The counts are summed as integers (per workgroup, then one integer atomic add per workgroup
 * onto a word a first launch zeroes); no floating-point atomics: two calls on the same tensors give identical bits.  No host
 * synchronisation, no allocation, no workspace.
 *
 * cfp_tsdf_raycast
 *   Inputs  Hd x Wd: the target grid K describes; t_min < t_max, both finite; step > 0; floor((t_max - t_min) / step) < 2^24.
 *   Ray     rx = ((float)x - cx) / fx,  ry = ((float)y - cy) / fy,  r = (rx, ry, 1): the ray parameter is the camera depth.  Samples at
 *           t_k = t_min + (float)k * step  for  k = 0 .. floorf((t_max - t_min) / step)  (a product, not a running sum).
 *   Point   q = (rx * t - T[3], ry * t - T[7], t - T[11]);  Pw = R^T q:  Xw = (T[0] * q.x + T[4] * q.y) + T[8] * q.z,  Yw with T[1], T[5],
 *           T[9],  Zw with T[2], T[6], T[10];  g = ((Xw - ox) / voxel, (Yw - oy) / voxel, (Zw - oz) / voxel).
 *   Sample  with i0 = floorf(g.x), a = g.x - i0 (j0, b and k0, c likewise): VALID iff 0 <= i0 <= Dx - 2, 0 <= j0 <= Dy - 2,
 *           0 <= k0 <= Dz - 2 (on the float values; NaN fails) and all 8 corners have Wt > 0.  Its value is the trilinear blend, x first,
 *           then y, then z:  c(j, k) = (1 - a) * F(i0, j, k) + a * F(i0 + 1, j, k);  e(k) = (1 - b) * c(j0, k) + b * c(j0 + 1, k);
 *           F = (1 - c) * e(k0) + c * e(k0 + 1).  The trilinear Wt is the same blend of the weights.
 *   Hit     the first pair of consecutive samples k - 1, k, both valid, with F_prev > 0 >= F_cur:
 *             depth = t_prev + step * (F_prev / (F_prev - F_cur))
 *           A consecutive valid pair with F_prev < 0 < F_cur met first is a back face: it ends the ray without a hit.  No hit: NaN.
 *   Std     1 / sqrtf(trilinear Wt) sampled at the ray's point at t = depth; NaN without a hit or where that sample is not valid.
 *   Normal  the central difference of the trilinear F at g +- 1 along each grid axis (+- one voxel along the world axes) at that
 *           point, n_w = (F(g + e_x) - F(g - e_x), ...), normalised (divided by sqrtf((x * x + y * y) + z * z)) and rotated into the
 *           camera frame, n = R n_w, rows left to right.  F falls from free space into the surface, so its gradient points out of the
 *           surface towards the camera that saw it: the sign convention of cfp_depth_unproject's normals (n . P < 0, a fronto-parallel
 *           wall gives (0, 0, -1)).  If one of the six samples is not valid, or the length is 0 or not finite, or there is no hit, the
 *           normal is (NaN, NaN, NaN) -- not the (0, 0, 0) of cfp_depth_unproject: a map knows where it knows nothing.
 *   Outputs depth [B,Hd,Wd] f32; normal [B,Hd,Wd,3] f32 or NULL; std [B,Hd,Wd] f32 or NULL.
 * One workgroup per 16 x 16 pixel tile; (F, Wt) is read as one 8-byte value.  The march may skip steps at which the ray cannot touch the
 * volume's box; the per-sample test still decides, so the result does not depend on it.  Reads only: bitwise reproducible.  No host
 * synchronisation, no allocation, no workspace. */
enum { CFP_TSDF_SEEN = 0, CFP_TSDF_UPDATED, CFP_TSDF_BEHIND };
int cfp_tsdf_integrate(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                       const float* std /* or NULL */, int Hu, int Wu, long long std_stride, float std_floor,
                       const float* K /* device, [B][4] */, const float* T /* device, [B][12] */,
                       float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, float ox, float oy, float oz, float voxel,
                       float trunc, float z_near, float w_max, int* counts /* [B][3] */, cfp_stream_t stream);
int cfp_tsdf_raycast(const float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz,
                     float voxel, const float* K /* device, [B][4] */, const float* T /* device, [B][12] */, int Hd, int Wd,
                     float t_min, float t_max, float step, float* depth /* [B][Hd][Wd] */, float* normal /* [B][Hd][Wd][3] or NULL */,
                     float* std /* [B][Hd][Wd] or NULL */, cfp_stream_t stream);

/* The map out of the volume: the zero crossings of F along the edges of the voxel lattice of a cfp_tsdf_integrate volume, as oriented
 * points in the WORLD frame.  Voxel (i, j, k) has index n = (k * Dy + j) * Dx + i and its centre at (ox + voxel * (float)i,
 * oy + voxel * (float)j, oz + voxel * (float)k), the expressions of cfp_tsdf_integrate.  Float32 in the order written here, no fused
 * multiply-add: every discrete decision is a comparison of float32 values in memory or one correctly rounded float32 operation.
 *   Candidates  edge e = 3 * n + a for axis a = 0 / 1 / 2 = +x / +y / +z runs from voxel p = n to q = p + e_a; candidates are numbered by
 *           e ascending (voxel-major, then axis).  An edge whose q is outside the grid is never kept.
 *   Kept    iff  Wt(p) > 0 && Wt(q) > 0 && Wt(p) >= w_min && Wt(q) >= w_min
 *           and  (F(p) < 0 && F(q) >= 0) || (F(p) >= 0 && F(q) < 0)          (-0.0 counts as non-negative, a NaN F never crosses)
 *           and  fabsf(F(p) - F(q)) <= max_jump                              (max_jump = +inf: no filter)
 *   Point   t = F(p) / (F(p) - F(q));  the coordinate along a is  o_a + voxel * ((float)idx_a + t),  the other two are the centre's.
 *   Std     1 / sqrtf((1 - t) * Wt(p) + t * Wt(q))
 *   Normal  the central difference of F at a voxel along axis c is F(+1) - F(-1), valid only if both neighbours are in the grid with
 *           Wt > 0;  g = (1 - t) * g(p) + t * g(q) per component;  len = sqrtf((gx * gx + gy * gy) + gz * gz);  n = g / len if all six
 *           differences are valid, len > 0 and len is finite, otherwise (NaN, NaN, NaN).  It points towards increasing F -- towards the
 *           free space the observing camera was in: the world-frame counterpart of the raycast's normal (R times it is what
 *           cfp_tsdf_raycast writes).
 *   Outputs per image, rows r < min(count, cap) in candidate order: points [B][cap][3] f32; normals [B][cap][3] f32 or NULL; std
 *           [B][cap] f32 or NULL; index [B][cap] i32 holding e; counts [B] i32: the true number kept, also when it exceeds cap.  Rows
 *           at or beyond min(count, cap) are not written.  points == NULL (then index, normals and std are NULL too): the call only
 *           counts.
 * Refused before anything is dereferenced: a null volume, counts or ws; points without index; normals or std without points;
 * non-positive dimensions; 3 * Dx * Dy * Dz >= 2^31 (the edge index is an int32) or B > 65535; a non-finite origin; voxel not positive
 * and finite; w_min or max_jump negative or NaN; cap < 1 with points; a volume or workspace that is not 8-byte aligned; a workspace
 * smaller than cfp_tsdf_surface_ws_bytes(B, Dx, Dy, Dz) (0 for arguments that make no sense).
 * Count per chunk of 256 voxels, exclusive scan per image in two levels, scatter -- four launches and no atomics: the order and every bit
 * are a function of the volume alone.  Nothing is zeroed (every word of the workspace is written before it is read).  No host
 * synchronisation, no allocation; capturable in a graph. */
size_t cfp_tsdf_surface_ws_bytes(int B, int Dx, int Dy, int Dz);
int cfp_tsdf_surface(const float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz,
                     float voxel, float w_min, float max_jump, int cap, float* points /* [B][cap][3] or NULL */,
                     float* normals /* [B][cap][3] or NULL */, float* std /* [B][cap] or NULL */, int* index /* [B][cap] or NULL */,
                     int* counts /* [B] */, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Colour in the map: a second volume next to the TSDF, fused by the same inverse-variance weights, and its two readers.  The conventions
 * are those of the TSDF block above: float32 in the order written here, no fused multiply-add, K [B][4] and T [B][12] ON THE DEVICE.
 *   Colour volume  float [B,Dz,Dy,Dx,4] ON THE DEVICE, 16-byte aligned: (R, G, B, Wc) per voxel, x fastest, next to the unchanged (F, Wt)
 *           volume.  Empty is (0, 0, 0, 0).  Wc is the colour's own inverse-variance sum, not Wt: frames integrated without an image
 *           (cfp_tsdf_integrate) and with one can be mixed freely, and the geometry never depends on whether colour is kept.
 *
 * cfp_tsdf_integrate_rgb
 *   Inputs  every argument of cfp_tsdf_integrate; rgb [B][3][H][W] f32 ON THE DEVICE, on the H x W grid, planar (the model's input);
 *           mean[3], cstd[3]: HOST arrays of finite floats, copied into the kernel arguments like cfp_render_rgb's; color: the colour
 *           volume; counts [B][4] i32 = {valid depth seen, updated, behind the surface, coloured}, overwritten.
 *   Voxel   everything cfp_tsdf_integrate does up to and including UPDATED, unchanged: (F, Wt) and the first three counts are bit for
 *           bit what cfp_tsdf_integrate writes for the same inputs.  Then, for an UPDATED voxel only, with the pix, w and sdf of the
 *           geometry step:  sdf > trunc: nothing (free space in front of the surface takes no colour);  otherwise
 *             c_k = rgb[b][k][pix] * cstd[k] + mean[k]  for k = 0, 1, 2;  skipped unless all three are finite;
 *             C_k' = (C_k * Wc + c_k * w) / (Wc + w)     Wc' = fminf(Wc + w, w_max)                                    COLOURED
 *           A voxel that is not coloured has its colour entry neither read nor written.
 *   Refused, with a message, before anything launches: everything cfp_tsdf_integrate refuses; a null rgb, mean, cstd or color; a
 *           non-finite mean or cstd; a colour volume that is not 16-byte aligned.
 * The same kernel as cfp_tsdf_integrate (its COLOR instance): integer counts onto words a first launch zeroes, no floating-point
 * atomics, two calls on the same tensors give identical bits; no host synchronisation, no allocation, no workspace; capturable.
 *
 * cfp_tsdf_shade: the colour of the map at the points a depth map names.
 *   Inputs  the colour volume; depth [B,Hd,Wd] f32 on the grid K describes -- a cfp_tsdf_raycast result, or any metric depth there.
 *   Pixel   the Ray rx, ry of cfp_tsdf_raycast, its Point at t = depth, and g, i0 / a, j0 / b, k0 / c of its Sample.  The result is
 *           (NaN, NaN, NaN) if the depth is not finite, if the cell test 0 <= i0 <= Dx - 2, 0 <= j0 <= Dy - 2, 0 <= k0 <= Dz - 2 fails (on
 *           the float values), or if no corner of the cell has Wc > 0.  Otherwise, over the corners in the order x fastest, then y, then
 *           z, with tw = (wx * wy) * wz (wx one of 1 - a and a, wy of 1 - b and b, wz of 1 - c and c):
 *             den = sum of tw, num_k = sum of tw * C_k, over the corners with Wc > 0, both accumulated in corner order from 0
 *             out_k = num_k / den
 *           The blend is renormalised over the corners that have a colour instead of demanding all eight: the colour band is trunc thick
 *           along the viewing ray, and corners of a hit cell may lie outside it at grazing angles.
 *   Outputs rgb_out [B,Hd,Wd,3] f32.
 * One thread per pixel in 16 x 16 tiles, a corner is one 16-byte load.  Reads only: bitwise reproducible.
 *
 * cfp_tsdf_surface_rgb: the colours of the rows cfp_tsdf_surface wrote.
 *   Inputs  both volumes; index [B][cap] i32, the edge indices e; counts [B] i32; cap >= 1.
 *   Row     for each r < min(counts[b], cap):  n = e / 3, a = e - 3 * n, p = n, q = p + e_a;  t = F(p) / (F(p) - F(q)), the expression of
 *           cfp_tsdf_surface, read from the geometry volume.  Both ends with Wc > 0: (1 - t) * C(p) + t * C(q) per channel; exactly one:
 *           that end's colour; neither: (NaN, NaN, NaN).  A row whose e is negative, is >= 3 * Dx * Dy * Dz, or whose q leaves the grid
 *           gets NaN and reads nothing: the index is device data and cannot take a load outside the volumes.
 *   Outputs colors [B][cap][3] f32; rows at or beyond min(count, cap) are not written.
 * Refused: null pointers; non-positive dimensions; 3 * Dx * Dy * Dz >= 2^31 or B > 65535; cap < 1; a geometry volume that is not 8-byte
 * or a colour volume that is not 16-byte aligned.  One thread per row; no workspace, no atomics, no host synchronisation. */
enum { CFP_TSDF_COLOURED = 3 };
int cfp_tsdf_integrate_rgb(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                           const float* std /* or NULL */, int Hu, int Wu, long long std_stride, float std_floor,
                           const float* K /* device, [B][4] */, const float* T /* device, [B][12] */,
                           float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, float ox, float oy, float oz, float voxel,
                           float trunc, float z_near, float w_max, const float* rgb /* device, [B][3][H][W] */,
                           const float* mean /* host, [3] */, const float* cstd /* host, [3] */,
                           float* color /* [B][Dz][Dy][Dx][4] */, int* counts /* [B][4] */, cfp_stream_t stream);
int cfp_tsdf_shade(const float* color /* [B][Dz][Dy][Dx][4] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz, float voxel,
                   const float* K /* device, [B][4] */, const float* T /* device, [B][12] */, int Hd, int Wd,
                   const float* depth /* [B][Hd][Wd] */, float* rgb_out /* [B][Hd][Wd][3] */, cfp_stream_t stream);
int cfp_tsdf_surface_rgb(const float* volume /* [B][Dz][Dy][Dx][2] */, const float* color /* [B][Dz][Dy][Dx][4] */, int Dx, int Dy, int Dz,
                         int B, const int* index /* [B][cap] */, const int* counts /* [B] */, int cap, float* colors /* [B][cap][3] */,
                         cfp_stream_t stream);

/* Camera tracking: one Gauss-Newton iteration of dense point-to-plane ICP of a frame against a model map, per image, without leaving the
 * device -- projective data association, the 6 x 6 normal equations weighted by the two variances, the solve and the pose update.  The
 * frame is the prediction and its std; the model is a depth / normal / std map in the MODEL camera: a cfp_tsdf_raycast (frame-to-model
 * tracking) or the previous frame's cfp_depth_unproject (frame-to-frame odometry).
 *   Inputs  pred [B,Hp,Wp] f32; H, W, interpolate, lo < hi as cfp_depth_unproject; std (NULL: none): image 0's Hu x Wu f32 plane, image
 *           b's std_stride ELEMENTS further, brought to H x W like the plane of cfp_depth_reproject; src_normals [B,H,W,3] f32 or NULL;
 *           K_src, K_mdl [B][4] f32 ON THE DEVICE: (fx, fy, cx, cy) of the H x W source grid and (fxm, fym, cxm, cym) of the Hm x Wm model
 *           grid, under the caller contract of cfp_depth_unproject; mdl_depth [B,Hm,Wm], mdl_normals [B,Hm,Wm,3], mdl_std [B,Hm,Wm] or NULL.
 *   Pose    T [B][12] f32 ON THE DEVICE, in and out: row-major [R|t], it takes a point of the CURRENT camera into the MODEL camera,
 *           Pm = R P + t, camera frames of cfp_depth_unproject.  The caller initialises it; the identity means the camera did not move.
 *   Pair    float32, in this order of operations (no fused multiply-add), for the source pixels x % stride == 0 && y % stride == 0:
 *             d = d(x, y) of cfp_depth_unproject (csrc/metrics_pred.h, bit for bit); skipped unless d is finite and d > 0
 *             P = (rx * d, ry * d, d)  with  rx = ((float)x - cx) / fx,  ry = ((float)y - cy) / fy
 *             X' = (T[0] * X + T[1] * Y) + T[2] * Z + T[3]      Y' likewise with T[4..7], Z' with T[8..11]   (left to right)
 *             skipped unless Z' is finite and Z' >= z_near;  u = fxm * (X' / Z') + cxm,  v = fym * (Y' / Z') + cym
 *             model pixel (xm, ym) = (floorf(u + 0.5f), floorf(v + 0.5f)), tested against 0 <= xm < Wm, 0 <= ym < Hm on the float
 *             values, before any conversion to int;  dm = mdl_depth there: skipped unless dm is finite and dm > 0;  n = mdl_normals
 *             there: skipped unless its three components are finite and (n.x * n.x + n.y * n.y) + n.z * n.z > 0.25f (a raycast writes
 *             NaN for "no normal", cfp_depth_unproject 0: both kinds of map work)
 *             Q = (((float)xm - cxm) / fxm * dm, ((float)ym - cym) / fym * dm, dm);  D = P' - Q
 *             skipped unless (D.x * D.x + D.y * D.y) + D.z * D.z <= dist_max * dist_max
 *             with src_normals: s = the source normal at the pixel, skipped unless s passes the test of n and
 *             ((R s) . n) >= cos_min, R s by rows left to right like P' without the translation, the dot product (a + b) + c
 *             r = (n.x * D.x + n.y * D.y) + n.z * D.z
 *             J = (P' x n, n) = (Y' * n.z - Z' * n.y, Z' * n.x - X' * n.z, X' * n.y - Y' * n.x, n.x, n.y, n.z): the derivative of r
 *             for a LEFT increment xi = (omega, v), P'' = exp(xi) P'
 *             w = 1 / (sf * sf + sm * sm):  sf = s > std_floor ? s : std_floor for s = the std plane at the pixel (a NaN s gives the
 *             floor; without a std plane sf = std_floor), sm = mdl_std at the model pixel, 0 when mdl_std is NULL or the value is not
 *             finite.  A pair whose w is 0 or not finite (an infinite std) is skipped.  With no std plane at all (both NULL) w = 1.
 *   Index   index [B,H,W] i32 or NULL: ym * Wm + xm of the pixel's pair, -1 where there is none; a pixel off the stride grid gets -1, so
 *           the map is fully written.
 *   Sums    30 per image, in this order: the 21 entries of the upper triangle of A = sum w J J^T by rows ((w * J[a]) * J[c], c >= a),
 *           the 6 of g = sum w J r ((w * J[a]) * r), sum (w * r) * r, sum w, the number of pairs.  Every product is float32, every
 *           accumulation double: per thread, __shfl_xor inside the wave, a fixed tree through LDS, ONE row of 30 doubles per workgroup
 *           in the workspace; the number of workgroups per image depends on the shape alone (at most 128).
 *   Step    one 64-lane workgroup per image, in double: the rows summed in a fixed order; sums [B][32] f64 or NULL receives the 30 values
 *           and 2 zeros.  A xi = -g is solved by LDL^T.  The step is REFUSED if pairs < min_pairs or a pivot is not above
 *           min_pivot * (largest diagonal entry of A); a refused step leaves T bit for bit as it was.  Otherwise exp(xi): with
 *           theta^2 = |omega|^2 and K = [omega]x,  Re = I + a K + b K^2,  te = (I + b K + c K^2) v,  a = sin(theta) / theta,
 *           b = (1 - cos(theta)) / theta^2,  c = (theta - sin(theta)) / theta^3, and (1, 1/2, 1/6) when theta^2 < 1e-12;
 *           T' = exp(xi) o T:  R' = Re R,  t' = Re t + te;  the rows of R' re-orthonormalised by Gram-Schmidt (row 0, row 1, row 2 =
 *           row 0 x row 1);  rounded to float32 and written over T.
 *   World   with T_ref [B][12] (camera-from-world of the model camera) T_world [B][12] is written on every call, refused or not: the
 *           camera-from-world pose of the current frame, R_cur = R^T R_ref, t_cur = R^T (t_ref - t) with [R|t] the T just written.
 *           T_ref and T_world are given together or not at all.
 *   Stats   stats [B][6] f32 = {pairs, sum w, sqrtf(sum w r r / sum w) (NaN without pairs), |omega|, |v| (0 when refused), accepted (1 / 0)}.
 *   Checks  stride >= 1; std_floor, z_near, dist_max positive and finite; 0 <= min_pivot < 1; min_pairs >= 6; -1 <= cos_min <= 1.
 * Two launches (accumulate, finalize) on `stream`, no atomics: two calls on the same inputs give identical bits.  No host
 * synchronisation, no allocation.  Workspace of cfp_icp_ws_bytes(B, H, W, stride) bytes, 8-byte aligned; 0 for arguments that make no sense. */
size_t cfp_icp_ws_bytes(int B, int H, int W, int stride);
int cfp_icp_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                 const float* std /* or NULL */, int Hu, int Wu, long long std_stride, float std_floor,
                 const float* src_normals /* [B][H][W][3] or NULL */, float cos_min, const float* K_src /* device, [B][4] */,
                 const float* mdl_depth /* [B][Hm][Wm] */, const float* mdl_normals /* [B][Hm][Wm][3] */,
                 const float* mdl_std /* [B][Hm][Wm] or NULL */, int Hm, int Wm, const float* K_mdl /* device, [B][4] */,
                 int stride, float z_near, float dist_max, int min_pairs, float min_pivot,
                 float* T /* device, [B][12], in and out */, const float* T_ref /* [B][12] or NULL */,
                 float* T_world /* [B][12] or NULL, given exactly when T_ref is */, int* index /* [B][H][W] or NULL */,
                 double* sums /* [B][32] or NULL */, float* stats /* [B][6] */, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Colour in camera tracking: the step of cfp_icp_step with a photometric term beside the point-to-plane one.  In front of a wall, a floor
 * or along a corridor geometry observes three of the six degrees of freedom and cfp_icp_step refuses; the texture on the surface observes
 * the other three.  The images are luminance planes: the frame's on the source grid, the model's on the model grid (the picture of the
 * map from the model camera: cfp_tsdf_shade of the raycast, or the previous frame's image).
 *
 * cfp_luma: one luminance plane out of an image.
 *   Inputs  layout 0: rgb [B,3,H,W] f32, the model's normalised planar input, with mean[3], cstd[3] ON THE HOST: c = rgb * cstd + mean per
 *           channel (the colour cfp_tsdf_integrate_rgb fuses).  Layout 1: rgb [B,H,W,3] f32 interleaved, already in 0..1 -- what
 *           cfp_tsdf_shade writes --, c = rgb; mean and cstd are not read.
 *   Pixel   Y = (0.299f * R + 0.587f * G) + 0.114f * B in float32 in that order (Rec. 601), no fused multiply-add; NaN if one of the three
 *           c is not finite (so the NaN of a shaded pixel without colour stays a NaN).
 *   Outputs luma [B,H,W] f32.
 * Refused: null pointers; another layout; layout 0 without mean and cstd, or with non-finite ones; non-positive dimensions; H * W >= 2^31
 * or B > 65535.  One pixel per lane; reads only its own pixel: bitwise reproducible; no workspace, no host synchronisation.
 *
 * cfp_icp_rgb_step: the arguments of cfp_icp_step, then src_luma [B,H,W] f32 (the H x W source grid), mdl_luma [B,Hm,Wm] f32,
 * photo_weight > 0 and finite, photo_max > 0 (+inf: no gate), residual [B,H,W] f32 or NULL.
 *   Geometric pair   the Pair of cfp_icp_step: the projection, the gates, w, r, J and the index map are its, bit for bit.
 *   Photometric pair a source pixel that has a geometric pair forms one as well when, with the u, v, X', Y', Z' of that pair (unrounded):
 *             x0 = floorf(u), y0 = floorf(v), ax = u - x0, ay = v - y0;  0 <= x0, x0 + 1 <= Wm - 1, 0 <= y0, y0 + 1 <= Hm - 1, tested on
 *             the float values so that NaN fails;  the four taps I00 = mdl_luma(x0, y0), I10 (x0 + 1, y0), I01 (x0, y0 + 1), I11 and
 *             Is = src_luma at the source pixel are finite;  in float32, in this order:
 *               top = I00 + ax * (I10 - I00)          bot = I01 + ax * (I11 - I01)          Im = top + ay * (bot - top)
 *               gx = (I10 - I00) + ay * ((I11 - I01) - (I10 - I00))          gy = bot - top
 *             -- the bilinear interpolant and its exact derivative in u and v --  rI = Im - Is,  and |rI| <= photo_max.
 *             gfx = gx * fxm, gfy = gy * fym;  a = (gfx / Z', gfy / Z', -((gfx * (X' / Z') + gfy * (Y' / Z')) / Z')): the gradient of Im in P'.
 *             JI = (P' x a, a) = (Y' * a.z - Z' * a.y, Z' * a.x - X' * a.z, X' * a.y - Y' * a.x, a.x, a.y, a.z): the derivative of rI
 *             for the LEFT increment of cfp_icp_step, J with n replaced by a.  The weight is wI = photo_weight for every pair
 *             (1 / sigma_I^2 for an intensity noise sigma_I, on the footing of w = 1 / variance of the depth).
 *   Residual  residual, when given, is fully written: rI where a photometric pair was formed, NaN elsewhere; a pixel off the stride grid
 *           gets NaN by the rule of `index`.
 *   Sums    60 per image: 0..29 the sums of cfp_icp_step over the geometric pairs; 30..59 in the same layout over the photometric
 *           pairs (21 of sum wI JI JI^T, 6 of sum wI JI rI, sum (wI * rI) * rI, sum wI, the count).  Float32 products, double
 *           accumulation, the fixed order of cfp_icp_step; ONE row of 60 doubles per workgroup in the workspace.
 *   Step    A = A_geo + A_photo, g = g_geo + g_photo, added in double; min_pairs is tested against the GEOMETRIC count, the pivot test
 *           runs on the combined A; the solve, exp, the composition, Gram-Schmidt and T_world are those of cfp_icp_step.  With no
 *           photometric pair at all (mdl_luma all NaN) T, T_world and the first six stats are bit for bit those of cfp_icp_step.
 *   Outputs sums [B][64] f64 or NULL: the 60 and 4 zeros.  stats [B][8] f32: the six of cfp_icp_step (pairs, sum w and the rms are the
 *           geometric ones), photo_pairs, photo_rms = sqrtf(sum wI rI rI / sum wI) (NaN without photometric pairs).
 *   Checks  those of cfp_icp_step; src_luma and mdl_luma are given together or not at all, and without them the call is refused
 *           (CFP_EINVAL): cfp_icp_step is the entry that tracks without an image.
 * One image level: the photometric term pulls over about half the finest texture period.  Two launches, no atomics: identical bits from
 * call to call; no host synchronisation, no allocation.  Workspace of cfp_icp_rgb_ws_bytes(B, H, W, stride) bytes, 8-byte aligned. */
int cfp_luma(const float* rgb, int layout, const float* mean /* host, [3], layout 0 */, const float* cstd /* host, [3], layout 0 */,
             int H, int W, int B, float* luma /* [B][H][W] */, cfp_stream_t stream);
size_t cfp_icp_rgb_ws_bytes(int B, int H, int W, int stride);
int cfp_icp_rgb_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                     const float* std /* or NULL */, int Hu, int Wu, long long std_stride, float std_floor,
                     const float* src_normals /* [B][H][W][3] or NULL */, float cos_min, const float* K_src /* device, [B][4] */,
                     const float* mdl_depth /* [B][Hm][Wm] */, const float* mdl_normals /* [B][Hm][Wm][3] */,
                     const float* mdl_std /* [B][Hm][Wm] or NULL */, int Hm, int Wm, const float* K_mdl /* device, [B][4] */,
                     int stride, float z_near, float dist_max, int min_pairs, float min_pivot,
                     float* T /* device, [B][12], in and out */, const float* T_ref /* [B][12] or NULL */,
                     float* T_world /* [B][12] or NULL, given exactly when T_ref is */, int* index /* [B][H][W] or NULL */,
                     double* sums /* [B][64] or NULL */, float* stats /* [B][8] */, void* ws, size_t ws_bytes,
                     const float* src_luma /* [B][H][W] */, const float* mdl_luma /* [B][Hm][Wm] */, float photo_weight,
                     float photo_max, float* residual /* [B][H][W] or NULL */, cfp_stream_t stream);

/* Surface-normal error of the predicted geometry against the ground truth's, per image, without leaving the device: the standard set of
 * the normal-estimation literature (mean, median and RMSE of the angle, share of pixels below 11.25, 22.5 and 30 degrees).
 *   Inputs  pred [B,Hp,Wp] f32 and gt [B,H,W] f32 (device); interpolate, lo < hi exactly as cfp_eval_metrics in mode 0; K [B][4] f32 ON
 *           THE DEVICE: (fx, fy, cx, cy) per image under the caller contract of cfp_depth_unproject (finite, fx and fy not 0).
 *   Depths  d_p(x, y) is the float32 value cfp_eval_metrics evaluates at the pixel in mode 0 (one implementation, csrc/metrics_pred.h:
 *           bit for bit); d_g(x, y) = gt[b][y][x].
 *   Normals n_p from d_p and n_g from d_g, both by the `Normal` of cfp_depth_unproject: clamped neighbours, the T_x / T_y form without
 *           cancellation, n = normalize(T_y x T_x), float32, no fused multiply-add, and (0, 0, 0) under the same rule (one of the five
 *           depths involved not finite, or a cross product of zero or non-finite length).  For the same five depths and intrinsics the
 *           three floats are the ones cfp_depth_unproject writes, bit for bit.
 *   Valid   a pixel counts iff the ground truth at the pixel and at its four clamped neighbours all satisfy lo < g < hi (a hole at 0
 *           next to a surface gives a meaningless tangent) and both normals are non-zero.  So H == 1 or W == 1 gives no valid pixel.
 *   Angle   float32, in this order, with p = n_p and g = n_g:
 *             c = (p.x * g.x + p.y * g.y) + p.z * g.z
 *             u = (p.y * g.z - p.z * g.y,  p.z * g.x - p.x * g.z,  p.x * g.y - p.y * g.x)      s = sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z)
 *             a = atan2f(s, c) * (float)(180 / pi)                                              degrees, 0 <= a <= 180
 *           Equal normals give exactly 0.  atan2 of (|cross|, dot) because acos(dot) loses half its digits near 0, where most pixels are.
 *   Histogram  1800 bins of 0.1 degree: k = min((int)(a * 10.0f), 1799); hist[b][k] counts the valid pixels (int32).
 *   out [B][7] f64 = {mean_deg, median_deg, rmse_deg, frac_11_25, frac_22_5, frac_30, n_valid} (CFP_NORMAL_*) with N = n_valid:
 *           mean_deg = (float64 sum of a) / N;  rmse_deg = sqrt((float64 sum of the float32 products a * a) / N);  the fractions count
 *           a < 11.25f, a < 22.5f, a < 30.0f;  median_deg = (k* + 0.5) * 0.1 with k* the smallest bin whose cumulative count reaches
 *           (N + 1) / 2 in integer division.  N == 0 gives NaN for the six metrics and n_valid = 0, as cfp_eval_metrics does.
 *   Optional outputs, each NULL to skip: hist [B][1800] i32; angle_map [B][H][W] f32 = a at the valid pixels, NaN elsewhere.  `out` is
 *           bit-identical with and without them.
 * Floating-point sums are float64 in a fixed order and never accumulated with atomics; the counts are integers (order-independent; LDS
 * and workspace integer atomics): two calls on the same tensors give identical bits.  No host synchronisation, no allocation; everything
 * runs on `stream` in the caller's workspace of cfp_normal_metrics_ws_bytes(B, H, W) bytes, 8-byte aligned; 0 for arguments that make
 * no sense. */
enum { CFP_NORMAL_MEAN = 0, CFP_NORMAL_MEDIAN, CFP_NORMAL_RMSE, CFP_NORMAL_FRAC_11_25, CFP_NORMAL_FRAC_22_5, CFP_NORMAL_FRAC_30,
       CFP_NORMAL_N_VALID };
size_t cfp_normal_metrics_ws_bytes(int B, int H, int W);
int cfp_normal_metrics(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo, float hi,
                       const float* K /* device, [B][4]: fx fy cx cy */, void* ws, size_t ws_bytes, double* out /* [B][7] */,
                       int* hist /* [B][1800] or NULL */, float* angle_map /* [B][H][W] or NULL */, cfp_stream_t stream);

/* Zone consistency: the ToF zones re-simulated from the PREDICTION and compared with what the sensor measured, per image, without leaving
 * the device -- the quality number that needs no ground truth.  On a rig the measurement is the sensor itself: per zone a rectangle, a
 * validity bit and the (mu, sigma) of its strongest return (the reference's `raw_data`, src/dataloader/zjuL5.py:106,148).  A ground-truth
 * map is perfectly consistent with its own cfp_tof_hist_sim: fed back with that call's rect, mask and fh it gives mu_p, sigma_p equal to
 * fh bit for bit and errors of exactly 0.
 *   Inputs  pred [B,Hp,Wp] f32; H, W, interpolate, lo < hi as cfp_eval_metrics in mode 0; rect [B,Z,4] f32 (sy, sx, ey, ex), mask [B,Z]
 *           u8 and raw [B,Z,2] f64 (the measured mu_m, sigma_m), read per image; max_distance, bins, bin_width, floor_count as
 *           cfp_tof_hist_sim, with the distance the measurement was made with.  All pointers are device pointers.
 *   Depth   d(y, x) is the float32 value cfp_eval_metrics evaluates at that pixel in mode 0: clip to [lo, hi] at model resolution, then
 *           the align-corners bilinear blend; interpolate = 0 requires equal sizes.  One implementation (csrc/metrics_pred.h): bit for bit.
 *   Zone    pixel (y, x) of the H x W grid belongs to zone z iff sy <= (float)y < ey && sx <= (float)x < ex, compared in float: the
 *           membership rule of cfp_eval_metrics_regions.  Rectangles may be non-square, of any size, overlapping (a pixel then counts in
 *           each) and partly or wholly off the image: only in-image pixels count.  An empty rectangle or a NaN coordinate gives an empty zone.
 *   Sensor  the model of cfp_tof_hist_sim applied to the zone's d, one implementation (csrc/tof_cluster.h): float32 histogram with
 *           bin = (int)(((d - 0.f) * (float)bins) / (max_distance - 0.f)), d == max_distance folded into the last bin, values outside
 *           [0, max_distance] and NaN ignored; bin 0 cleared and floor_count subtracted, clamped at 0; the strongest run of consecutive
 *           non-zero bins kept, lowest start winning ties; n, mu, sigma in float64 over the bin centres
 *           ((double)(float)((j+1)*bin_width) + j*bin_width)/2 in ascending bin order with the divisor (double)((float)n + 1e-9f) and
 *           sigma = sqrt(var/nf) + 1e-9.  No return (n = 0) gives mu = 0 and sigma = 1e-9.
 *   Window  in float64 from the measured inputs: w = 3*sigma_m if 3*sigma_m > bin_width else bin_width (so a NaN sigma_m gives bin_width);
 *           a pixel is inside iff mu_m - w <= (double)d <= mu_m + w.
 *   zone [B][Z][6] f64 = {mu_p, sigma_p, n_signal, n_pix, n_window, state}: mu_p, sigma_p and n_signal = n of the sensor model; n_pix the
 *           in-image pixels of the rectangle; n_window the ones inside the window, 0 when mask == 0; state
 *             0 compared     mask != 0 and n_signal > 0
 *             1 lost         mask != 0 and the prediction has no return
 *             2 unmeasured   mask == 0 and the prediction has a return (not an error: a dropped zone looks like this)
 *             3 neither
 *   summary [B][10] f64 = {n_compared, mae_mu, rmse_mu, rel_mu, mae_sigma, frac_1bin, frac_window, n_lost, n_unmeasured, n_measured}
 *           (CFP_ZONE_*).  Over the set C of compared zones: mae_mu = mean |mu_p - mu_m|, rmse_mu = sqrt(mean (mu_p - mu_m)^2),
 *           rel_mu = mean |mu_p - mu_m| / mu_m, mae_sigma = mean |sigma_p - sigma_m|, frac_1bin = the share with |mu_p - mu_m| <= bin_width;
 *           the five are NaN when n_compared == 0.  frac_window = sum n_window / sum n_pix over the zones with mask != 0, NaN if that
 *           pixel sum is 0.  n_lost, n_unmeasured count states 1 and 2; n_measured the zones with mask != 0.
 *   dev_map [B][H][W] f32 or NULL (skipped): d - (float)mu_m of the lowest-index zone with mask != 0 that contains the pixel, NaN where
 *           there is none.  zone and summary are bit-identical with and without it.
 * Three launches on `stream` -- one workgroup per (image, zone), one per image over the zone table in a fixed summation order, one lane per
 * pixel for the map -- with no workspace, no host synchronisation, no global atomics and no floating-point atomics (integer LDS atomics
 * only): two calls on the same tensors give identical bits.  CFP_ESHAPE for B*Z >= 2^31 or an image of 2^31 pixels or more. */
enum { CFP_ZONE_N_COMPARED = 0, CFP_ZONE_MAE_MU, CFP_ZONE_RMSE_MU, CFP_ZONE_REL_MU, CFP_ZONE_MAE_SIGMA, CFP_ZONE_FRAC_1BIN,
       CFP_ZONE_FRAC_WINDOW, CFP_ZONE_N_LOST, CFP_ZONE_N_UNMEASURED, CFP_ZONE_N_MEASURED };
enum { CFP_ZONE_COMPARED = 0, CFP_ZONE_LOST, CFP_ZONE_UNMEASURED, CFP_ZONE_NEITHER };
int cfp_tof_zone_consistency(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                             const float* rect /* [B][Z][4] sy sx ey ex */, const unsigned char* mask /* [B][Z] */,
                             const double* raw /* [B][Z][2] measured mu, sigma */, int Z,
                             float max_distance, int bins, double bin_width, int floor_count,
                             double* zone /* [B][Z][6] */, double* summary /* [B][10] */,
                             float* dev_map /* [B][H][W] or NULL */, cfp_stream_t stream);

/* Zone-consistency loss: cfp_tof_zone_consistency turned into a training objective with a gradient on the prediction, on the device --
 * the term that needs no ground truth (`train.py --w_zone`).  Everything up to the strongest run is the metric's, bit for bit, from the
 * same code (csrc/metrics_pred.h, csrc/tof_cluster.h); the arguments up to floor_count are the metric's.
 *   Depth     d_i is the depth at pixel i of the H x W grid: the float32 value of cfp_tof_zone_consistency (mode 0 with (lo, hi): the taps
 *             clipped at model resolution, then the align-corners blend in float32).
 *   Pixels    the pixels of zone z are those of the metric: sy <= (float)y < ey && sx <= (float)x < ex, in-image pixels only.
 *   Counts    cnt_j is the zone's histogram of bin(d_i) (the metric's float32 bin); c'_j the histogram after the floor (bin 0 cleared,
 *             floor_count subtracted, clamped at 0); [a, b) the strongest run of consecutive non-zero c'_j, lowest start winning ties;
 *             n_z = sum_{j in [a,b)} c'_j.
 *   Weights   omega_j = c'_j / cnt_j for j in [a, b), 0 elsewhere.
 *   Zone mean m_z = (1/n_z) sum_{i in zone} omega_{bin(d_i)} * d_i, accumulated in float64 over the float32 d_i; 0 when n_z = 0.  The
 *             sensor model's mu weights the bin centres by the floored counts, so m_z uses the same weights: |m_z - mu_z| <= bin_width/2
 *             for any floor, which the unweighted mean of the run's pixels does not keep.
 *   Compared  a zone is compared when mask != 0, n_z > 0 and the measured mu_m (raw[b][z][0]) is finite; n_b is their number in image b.
 *             The sigma column of raw is not used.
 *   Residual  r_z = m_z - mu_m.
 *   Dead zone e_z = max(|r_z| - bin_width/2, 0): the sensor cannot tell depths apart inside its bin.
 *   Penalty   Huber: rho_z = e_z^2 / (2 delta) if e_z <= delta, else e_z - delta/2; delta > 0 and finite (CFP_EINVAL otherwise).
 *   Loss      L_b = (1/n_b) sum_{compared z} rho_z, and n_b = 0 contributes 0;  L = (1/B) sum_b L_b.
 *   Gradient  with the run and the weights held constant:
 *               dL/dd_i = sum_{z contains i, compared} grad_scale * min(e_z/delta, 1) * sgn(r_z) * omega_{bin(d_i)} / (B * n_b * n_z),
 *             carried to pred through the transpose of the blend, times [lo <= pred_t <= hi] per tap t: the derivative of the clip,
 *             closed interval, as torch.clamp.  A NaN d_i has no bin and no gradient; a tap outside the clip interval gets 0, NaN and
 *             Inf included: the gradient this call produces is finite wherever the inputs are not, and L is finite.
 *   ws        cfp_tof_zone_loss_ws_bytes(B, Z, bins) bytes (0 for arguments the call refuses), 16-byte aligned: omega_j / n_z per
 *             (image, zone, bin).  CFP_EINVAL when null, misaligned or too small.
 *   zone [B][Z][8] f64 = {m_z, n_z, r_z, rho_z, run_start, run_stop, state, coef}: run_start = a, run_stop = b (both = bins when
 *             n_z = 0); state as cfp_tof_zone_consistency (CFP_ZONE_COMPARED ... from mask and n_z alone: a zone with state 0 and a
 *             non-finite mu_m is not compared); r_z is NaN, rho_z and coef are 0 for a zone that is not compared;
 *             coef = grad_scale * min(e_z/delta, 1) * sgn(r_z) / (B * n_b) = d(grad_scale * L)/dm_z.
 *   out [1+B] f32 = L, then the L_b (L is the float64 mean of the float32 L_b).
 *   grad_pred [B][Hp][Wp] f32 or NULL (value only: out and zone are the same bits).  accumulate = 0 writes every element, accumulate = 1
 *             adds to what is there (one float32 addition per element), so a step needs no add launch after the SILog backward.
 * Three launches on `stream` (two without grad_pred): one workgroup per (image, zone); one workgroup over the zone table in a fixed
 * order; a gather over the pred grid, one lane per pixel, in which overlapping zones sum in index order in float64.  No host
 * synchronisation, no global atomics and no floating-point atomics (integer LDS atomics only): two calls on the same tensors give
 * identical bits.  CFP_ESHAPE for bins outside 1..1024, B*Z >= 2^31 or an image of 2^31 pixels or more. */
size_t cfp_tof_zone_loss_ws_bytes(int B, int Z, int bins);
int cfp_tof_zone_loss(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                      const float* rect /* [B][Z][4] sy sx ey ex */, const unsigned char* mask /* [B][Z] */,
                      const double* raw /* [B][Z][2] measured mu, sigma */, int Z,
                      float max_distance, int bins, double bin_width, int floor_count,
                      double delta, float grad_scale, int accumulate, void* ws, size_t ws_bytes,
                      double* zone /* [B][Z][8] */, float* out /* [1+B] */, float* grad_pred /* [B][Hp][Wp] or NULL */,
                      cfp_stream_t stream);

/* Pictures on the device: what the reference's `colorize` (src/utils/utils.py:44-64) paints on the host after moving the prediction
 * there, defined on the value the metrics evaluate.  Three entry points, one launch each; no workspace, no atomics, no host
 * synchronisation, capturable in a graph.  Every float32 operation below is rounded once (no fused multiply-add).
 *   Output addressing, shared: out is uint8, channel c (0 red, 1 green, 2 blue) of pixel (b, y, x) lies at
 *           out[b * image_stride + (y * pitch + x) * 3 + c]; pitch >= W in PIXELS, image_stride >= H * pitch * 3 in BYTES (CFP_ESHAPE
 *           otherwise), so a caller renders into a sub-rectangle of a larger canvas by offsetting the base pointer.  Any byte alignment
 *           is accepted: when base % 4 == 0, image_stride % 4 == 0 and pitch % 4 == 0 a lane stores the 12 bytes of 4 consecutive
 *           pixels as whole dwords, otherwise -- and for the W % 4 tail of a row -- bytes; both give the same bytes.  Bytes outside the
 *           H x W rectangle are never read or written.
 *   Lookup  colour of a value v under (vmin, vmax, lut), lut [256][3] uint8 on the device -- matplotlib's rule for float input with
 *           bytes=True:  t = (v - vmin) / (vmax - vmin) * 256.f;  NaN -> (0, 0, 0) (the "bad" colour);  t < 0 -> lut[0];
 *           t >= 256 -> lut[255];  otherwise lut[(int)t].  vmin < vmax, both finite (CFP_EINVAL otherwise).
 *
 * cfp_render_depth: the prediction, the ground truth or their error as a picture and / or as 16-bit integers.
 *   d       the float32 value cfp_eval_metrics and cfp_depth_unproject see at the pixel in mode 0 (evaluate_all.py:40-41): clip to
 *           [lo, hi] at model resolution, then the align-corners bilinear blend; interpolate = 0 needs equal sizes.  One implementation
 *           (csrc/metrics_pred.h): bit for bit.  valid means lo < gt < hi.
 *   what    CFP_RENDER_DEPTH    v = d                     every pixel painted     gt may be NULL
 *           CFP_RENDER_GT       v = gt                    painted iff valid       pred may be NULL (Hp, Wp, interpolate are ignored)
 *           CFP_RENDER_ABS_ERR  v = fabsf(d - gt)         painted iff valid
 *           CFP_RENDER_REL_ERR  v = fabsf(d - gt) / gt    painted iff valid
 *           A painted pixel gets the lookup of v, an unpainted one (255, 255, 255) -- the invalid colour of `colorize`, utils.py:60.
 *   u16_out optional, [B][H][W] contiguous uint16, with DEPTH and GT only:  m = v * u16_scale;  NaN or m <= 0 -> 0;
 *           m >= 65535 -> 65535;  otherwise (uint16_t)rintf(m), ties to even;  an unpainted pixel -> 0.  u16_scale finite and > 0;
 *           1000 gives the 16-bit millimetre PNG of NYU / BTS.  Whole dwords when the base is 4-byte aligned and W is even.
 *   out may be NULL when u16_out is given (lut, vmin, vmax, image_stride and pitch are then ignored); both NULL is CFP_EINVAL. */
enum { CFP_RENDER_DEPTH = 0, CFP_RENDER_GT = 1, CFP_RENDER_ABS_ERR = 2, CFP_RENDER_REL_ERR = 3 };
int cfp_render_depth(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo, float hi,
                     int what, float vmin, float vmax, const unsigned char* lut /* [256][3] */, unsigned char* out,
                     long long image_stride, int pitch, unsigned short* u16_out /* [B][H][W] or NULL */, float u16_scale,
                     cfp_stream_t stream);
/* cfp_render_zones: the ToF input drawn over what `out` already holds.  hist [B][Z][S] f32 (the depth samples of a zone, the model's
 * hist_data), rect [B][Z][4] f32 (sy, sx, ey, ex), mask [B][Z] u8, 1 <= Z <= 256, S >= 1 (CFP_ESHAPE otherwise).
 *   Zone    pixel (y, x) belongs to the FIRST zone z in index order with sy <= y < ey && sx <= x < ex, compared in float: the
 *           membership rule of cfp_eval_metrics_regions.  A pixel in no zone is left untouched.
 *   Colour  c = (0, 0, 0) on the zone's one-pixel border, y < sy + 1 || y >= ey - 1 || x < sx + 1 || x >= ex - 1;  else
 *           (128, 128, 128) if mask[b][z] == 0;  else the lookup of v = (hist[b][z][0] + ... + hist[b][z][S-1]) / S, summed in index
 *           order in float32.
 *   Blend   per channel, in integers: out = (c * alpha + out * (256 - alpha) + 128) >> 8, alpha 0 .. 256 (256 is opaque, 0 changes
 *           nothing; CFP_EINVAL otherwise). */
int cfp_render_zones(const float* hist /* [B][Z][S] */, const float* rect /* [B][Z][4] */, const unsigned char* mask /* [B][Z] */,
                     int Z, int S, int H, int W, int B, float vmin, float vmax, const unsigned char* lut /* [256][3] */, int alpha,
                     unsigned char* out, long long image_stride, int pitch, cfp_stream_t stream);
/* cfp_render_rgb: the normalised colour image back to bytes.  rgb [B][3][H][W] f32 on the device; mean, std: HOST arrays of 3 finite
 * floats, copied into the kernel arguments.  Per channel c:  v = x * std[c] + mean[c];  NaN or v <= 0 -> 0;  v >= 1 -> 255;  otherwise
 * (uint8_t)rintf(v * 255.f). */
int cfp_render_rgb(const float* rgb /* [B][3][H][W] */, const float* mean /* host, [3] */, const float* std /* host, [3] */, int H,
                   int W, int B, unsigned char* out, long long image_stride, int pitch, cfp_stream_t stream);

/* ---- training-step kernels: backward of the dense convolution, batch-statistics BatchNorm --------------------------
 * (the training row of SURVEY.md section 8: cfpnet_amd/autograd_hip.py chains them into the backward of the whole network) */

/* Weight gradient of nn.Conv2d / nn.Linear (autograd of the layers cfp_conv2d_nhwc replaces; train.py:125):
 * dw[Cout][KH*KW*Cin] (f32) = beta * dw + sum over output pixels of dy[m][co] * x[window(m)][ci].  x [B,H,W,Cin] and
 * dy [B,Ho,Wo,Cout] in `dtype` (16-bit inputs are widened to f32 on the way to the matrix cores; accumulation f32).
 * dtype CFP_F32X3 (also for _bias without db, and _deferred): float32 x / dy in split precision, see cfp_conv2d_wgrad_x3.
 * Split over pixel chunks into f32 slabs (ws) that a second kernel adds in a fixed order: bit-reproducible. */
size_t cfp_conv2d_wgrad_ws_bytes(int Cout, int K, int M);
int cfp_conv2d_wgrad(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, int B, int H, int W, int Cin, int Cout,
                     int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, float beta, int dtype, void* ws,
                     size_t ws_bytes, cfp_stream_t stream);
/* The same, plus the bias gradient db[co] = beta_b * db + sum over output pixels of dY[m][co] from the SAME launch (16-bit dtypes only:
 * one more matrix-core product against a fragment of ones; float32 callers use cfp_colsum).  db may be NULL (= cfp_conv2d_wgrad). */
int cfp_conv2d_wgrad_bias(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, float* db, int B, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, float beta, float beta_b,
                          int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);
/* The reduction of the slabs postponed and batched: cfp_conv2d_wgrad_deferred runs the slab launch of cfp_conv2d_wgrad_bias and
 * describes the remaining reduction in *job (host memory; job->nsplit = 0 when the launch already wrote dw in place) instead of
 * launching it; cfp_wgrad_reduce_jobs(jobs, n) then finishes up to 48 layers per launch (the job table travels in the kernel
 * arguments), in the same summation order as the per-layer reduction: bit-identical gradients, ~240 launches fewer per training
 * step.  `ws` of a deferred call must stay untouched until its job has been reduced; jobs that write the same dw / db are put
 * into separate launches, in the order given. */
typedef struct cfp_wgrad_job {
  const float* slabs; float* dw; float* db;
  long long n, n_dw;
  int nsplit, ew;
  float beta, beta_b;
} cfp_wgrad_job;
int cfp_conv2d_wgrad_deferred(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, float* db, int B, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, float beta, float beta_b,
                              int dtype, void* ws, size_t ws_bytes, cfp_wgrad_job* job, cfp_stream_t stream);
int cfp_wgrad_reduce_jobs(const cfp_wgrad_job* jobs, int njobs, cfp_stream_t stream);
/* Two more producers of such jobs (their finishing sums are [split][n] slabs too): the depthwise 3x3 weight gradient
 * (cfp_dwconv3x3_wgrad) and the LayerNorm parameter gradients (cfp_layernorm_bwd: dbeta | dgamma).  Same contract: `ws` untouched
 * until cfp_wgrad_reduce_jobs has run; the results equal the immediate calls up to float32 summation order. */
int cfp_dwconv3x3_wgrad_deferred(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, int B, int H, int W, int C, int stride,
                                 int pad_t, int pad_l, int Ho, int Wo, float beta, int dtype, void* ws, size_t ws_bytes,
                                 cfp_wgrad_job* job, cfp_stream_t stream);
int cfp_layernorm_bwd_deferred(const void* x, int ld, const void* dy, int dy_ld, const float* gamma, float eps, void* dx, int dx_ld,
                               int accumulate, float* dgamma, float* dbeta, long long rows, int C, int dtype, void* ws, size_t ws_bytes,
                               cfp_wgrad_job* job, cfp_stream_t stream);
/* wt[Cin][KH][KW][Cout] = w[Cout][KH-1-kh][KW-1-kw][Cin]: the weights the data gradient convolves with. */
int cfp_conv2d_weight_flip(const void* w, void* wt, int Cout, int KH, int KW, int Cin, int dtype, cfp_stream_t stream);
/* The same for n weight tensors in one launch (a training step flips every convolution's weights once).  `desc` is a DEVICE
 * array of n rows of 8 int64: {source offset, destination offset (elements from src_base / dst_base), Cout, KH, KW, Cin,
 * first workgroup, workgroups}; a tensor of E elements takes cfp_weight_flip_blocks(E) workgroups, rows sorted by first
 * workgroup, total_blocks = their sum. */
int cfp_weight_flip_blocks(long long elems);
int cfp_conv2d_weight_flip_batch(const void* src_base, void* dst_base, const long long* desc, int n, int total_blocks, int dtype,
                                 cfp_stream_t stream);
/* Data gradient: dx [B,H,W,Cin] (+= when accumulate) from dy [B,Ho,Wo,Cout] and the flipped weights, for the forward
 * geometry (KH,KW,stride,pad_t,pad_l): a stride-1 convolution over dy with `stride - 1` zeros stuffed between its pixels.
 * dtype CFP_F32X3: float32 dy / dx, f16x3 matrix math; `wt` is then the PRE-SPLIT operand of the flipped weights
 * (cfp_pack_w_x3_batch mode 1, = cfp_pack_w_x3 of cfp_conv2d_weight_flip's output) and stride > 1 needs `ws` of
 * cfp_conv2d_dgrad_x3_ws_bytes (a zero-stuffed copy of dy). */
int cfp_conv2d_dgrad(const void* dy, int dy_ld, const void* wt, void* dx, int dx_ld, int B, int H, int W, int Cin, int Cout,
                     int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate, int dtype, void* ws,
                     size_t ws_bytes, cfp_stream_t stream);

/* ---- f16x3 training numerics (float32 tensors, split-precision matrix math in the dense-convolution backward) ----------------
 * Activation gradients are far below the range of IEEE half (SILog spreads ~10 / pixels over the image), so the dY operand of both
 * backward GEMMs carries a power-of-two scale: cfp_grad_absmax leaves the float32 bits of max|dY| in one device int32 (`dy_scale`);
 * the GEMMs multiply dY by 2^e before the split (e = 14 - exponent of the maximum: max * 2^e in [2^14, 2^15)) and multiply their
 * float32 results by 2^-e.  Both multiplications are exact, so dY * 2^k gives results * 2^k bit for bit.  dy_scale NULL: e = 0. */
int cfp_grad_absmax(const float* x, int ld, long long rows, int C, int* dy_scale, cfp_stream_t stream);
/* out [B][(Ho-1)*dil+1][(Wo-1)*dil+1][C] (contiguous) = dy * 2^e with dil - 1 zero pixels between dy's pixels (dil = 1: a scaled copy),
 * inv[0 .. n_inv) = 2^-e (the epilogue scale of the convolution that reads `out`). */
int cfp_grad_scale(const float* dy, int ld, int B, int Ho, int Wo, int C, int dil, const int* dy_scale, float* out, float* inv, int n_inv,
                   cfp_stream_t stream);
/* Weight gradient in f16x3 (the call cfp_conv2d_wgrad / _deferred make for dtype CFP_F32X3, plus the dY scale): float32 x and dy,
 * both split into hi / lo halves in the loader, three v_mfma_f32_16x16x32_f16 per block, float32 slabs reduced as for float32
 * (job != NULL: deferred as cfp_conv2d_wgrad_deferred; ws of cfp_conv2d_wgrad_ws_bytes).  The bias gradient stays cfp_colsum. */
int cfp_conv2d_wgrad_x3(const float* x, int x_ld, const float* dy, int dy_ld, float* dw, int B, int H, int W, int Cin, int Cout,
                        int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, float beta, const int* dy_scale, void* ws,
                        size_t ws_bytes, cfp_wgrad_job* job, cfp_stream_t stream);
/* Data gradient in f16x3 with the dY scale: dx = conv(dy) + res (res may be NULL or equal dx: accumulation); geometry and `wt` as
 * cfp_conv2d_dgrad with CFP_F32X3.  With a scale or stride > 1, `ws` of cfp_conv2d_dgrad_x3_ws_bytes holds the scaled (stuffed) dy. */
size_t cfp_conv2d_dgrad_x3_ws_bytes(int B, int Ho, int Wo, int Cout, int Cin, int stride);
int cfp_conv2d_dgrad_x3(const float* dy, int dy_ld, const void* wt, const float* res, int res_ld, float* dx, int dx_ld, int B, int H, int W,
                        int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, const int* dy_scale,
                        void* ws, size_t ws_bytes, cfp_stream_t stream);
/* Every convolution's pre-split operands of a training step in one launch.  `desc` is a DEVICE array of n rows of 8 int64:
 * {source offset (floats from src_base), destination offset (halves from dst_base), Cout, KH, KW, Cin, first workgroup, mode};
 * mode 0 writes cfp_pack_w_x3 of w [Cout][KH*KW*Cin], mode 1 cfp_pack_w_x3 of its cfp_conv2d_weight_flip ([Cin][KH*KW*Cout]),
 * bit for bit.  A tensor takes cfp_pack_w_x3_blocks(rows, K) workgroups (rows / K of the packed matrix), rows sorted by first
 * workgroup, total_blocks = their sum. */
int cfp_pack_w_x3_blocks(long long rows, int K);
int cfp_pack_w_x3_batch(const float* src_base, void* dst_base, const long long* desc, int n, int total_blocks, cfp_stream_t stream);

/* cfp_conv2d_nhwc (no activation / residual) that ALSO emits, per tile of output rows, the channel moments of its stored output for the
 * batch-statistics BatchNorm that follows it in model.train() (timm ConvBnAct / torch `Conv2d -> BatchNorm2d`): mom[tile][0][c] = mean,
 * mom[tile][1][c] = sum of squared deviations from that mean, over the tile's rows.  On return *nsplit = tiles written and
 * *rows_per_split = rows per tile -- or *nsplit = 0 when the kernel chosen for this problem does not produce them (float32, split-K,
 * mom_floats too small): then run cfp_bn_train_stats.  Saves one pass over the activation and one launch per layer. */
int cfp_conv2d_nhwc_moments(const void* in, int in_ld, const void* w, const float* bias, void* out, int out_ld, int B, int H, int W,
                            int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int dtype,
                            void* ws, size_t ws_bytes, float* mom, size_t mom_floats, int* nsplit, int* rows_per_split,
                            cfp_stream_t stream);
/* cfp_bn_train_stats from such partials ([split][2][C]; split j covers rows [j * rows_per_split, min(rows, (j + 1) * rows_per_split))). */
int cfp_bn_train_stats_partials(const float* partial, int nsplit, long long rows, long long rows_per_split, int C, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                                float* var, float* invstd, float* scale, float* shift, cfp_stream_t stream);

/* Training-mode BatchNorm over `rows` NHWC rows (nn.BatchNorm2d/1d in model.train()): batch mean / biased variance
 * (one pass: shifted sums merged as exact (n, mean, M2) triples), running statistics updated with `momentum` (running_var from the unbiased variance), and the folded
 * per-channel scale = gamma*invstd, shift = beta - mean*scale that cfp_scale_shift_act applies with the activation. */
size_t cfp_bn_ws_bytes(int C);
int cfp_bn_train_stats(const void* x, int ld, long long rows, int C, int dtype, const float* gamma, const float* beta, float eps,
                       float momentum, float* running_mean, float* running_var, float* mean, float* var, float* invstd,
                       float* scale, float* shift, void* ws, size_t ws_bytes, cfp_stream_t stream);
/* out = act(x * scale[c] + shift[c]) (BatchNorm apply + SiLU / LeakyReLU / ReLU / GELU / sigmoid / none). */
int cfp_scale_shift_act(const void* x, int ld, const float* scale, const float* shift, int act, void* out, int out_ld,
                        long long rows, int C, int dtype, cfp_stream_t stream);
/* out = act(x * scale[c] + shift[c]) + res  (res may be NULL): the block's skip connection added in the same pass (the sum is rounded
 * like the separate add of the stored activation). */
int cfp_scale_shift_act_res(const void* x, int ld, const float* scale, const float* shift, int act, const void* res, int res_ld,
                            void* out, int out_ld, long long rows, int C, int dtype, cfp_stream_t stream);
/* Backward of act(BatchNorm(x)) in training mode: dgamma, dbeta (f32) and dx from the pre-BN input x and dy. */
int cfp_bn_train_bwd(const void* x, int ld, const void* dy, int dy_ld, long long rows, int C, int dtype, const float* mean,
                     const float* invstd, const float* scale, const float* shift, int act, float* dgamma, float* dbeta,
                     void* dx, int dx_ld, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* out[c] = sum over rows of x[r][c] (f32): the bias gradient of a conv / linear layer.  ws: cfp_bn_ws_bytes(C). */
int cfp_colsum(const void* x, int ld, long long rows, int C, int dtype, float* out, void* ws, size_t ws_bytes, cfp_stream_t stream);
/* dz = dy * act'(z): backward of a stand-alone SiLU / ReLU / LeakyReLU / GELU / sigmoid given its input z. */
int cfp_act_bwd(const void* z, int ld, const void* dy, int dy_ld, int act, void* dz, int dz_ld, long long rows, int C, int dtype,
                cfp_stream_t stream);
/* Backward of nn.LayerNorm over the channel axis (transformer.py:38-39, convnext.py:31): dx (+= when accumulate),
 * dgamma, dbeta (f32) from the layer's input x and dy. */
size_t cfp_layernorm_bwd_ws_bytes(long long rows, int C);
int cfp_layernorm_bwd(const void* x, int ld, const void* dy, int dy_ld, const float* gamma, float eps, void* dx, int dx_ld,
                      int accumulate, float* dgamma, float* dbeta, long long rows, int C, int dtype, void* ws, size_t ws_bytes,
                      cfp_stream_t stream);

/* out = a*x + b*y (y may be NULL): gradient accumulation at skip connections, scaling. */
int cfp_axpby(const void* x, int x_ld, const void* y, int y_ld, float a, float b, void* out, int out_ld, long long rows, int C,
              int dtype, cfp_stream_t stream);
/* Gradient of `x + PE[oy:oy+H, ox:ox+W]` (fusion.py:87-97) w.r.t. the learned table: dtable[...] = beta*dtable + sum_b dx. */
int cfp_rowtable_grad(const void* dx, int ld, float* dtable, int B, int H, int W, int C, int Wt, int oy, int ox, float beta,
                      int dtype, cfp_stream_t stream);
/* Squeeze-excite gate in the training step (timm SqueezeExcite of the encoder's inverted-residual blocks, encoder.py:57-69), float32:
 *   forward : mean[b,c] = sum_s partial[b,s,c] * inv_hw;  z1 = W1 mean + b1;  gate = sigmoid(W2 silu(z1) + b2)      (one launch)
 *   backward: from dgate[b,c] = sum_hw dy * x (cfp_channel_dot): dW1, db1, dW2, db2 (out = beta * out + grad) and
 *             add[b,c] = d(loss)/d(mean) * inv_hw, the term cfp_bcast_fma adds to dy * gate                          (two launches)
 * W1 [Rp][C], b1 [Rp], W2 [C][Rp], b2 [C]; Rp = hidden width padded to a multiple of 4 with zero rows / columns, <= 64; C <= 2048;
 * B <= 64 in the backward.  mean [B][C], z1 [B][Rp], gate [B][C] are kept by the caller between the two calls;
 * ws: cfp_se_train_ws_floats(B, C, Rp) floats. */
size_t cfp_se_train_ws_floats(int B, int C, int Rp);
int cfp_se_train_fwd(const float* partial, int nsplit, float inv_hw, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* mean, float* z1, float* gate, int B, int C, int Rp, cfp_stream_t stream);
int cfp_se_train_bwd(const float* dgate, const float* gate, const float* z1, const float* mean, const float* w1, const float* w2,
                     float* dw1, float* db1, float* dw2, float* db2, float* add, float* ws, float inv_hw, float beta, int B, int C,
                     int Rp, cfp_stream_t stream);
/* out[b][c] = sum over the HW rows of image b of x*y: gradient of the squeeze-excite gate (sum dy * x). */
int cfp_channel_dot(const void* x, int x_ld, const void* y, int y_ld, float* out, int B, int HW, int C, int dtype, cfp_stream_t stream);
/* dx = dy * gate[b][c] + add[b][c] (add may be NULL): squeeze-excite backward w.r.t. the gated activation. */
int cfp_bcast_fma(const void* dy, int dy_ld, const float* gate, const float* add, void* dx, int dx_ld, int B, int HW, int C, int dtype,
                  cfp_stream_t stream);
/* Depthwise 3x3 backward (conv_dw of timm's InvertedResidual): data gradient (+= when accumulate) and weight gradient
 * dw[9][C] f32 = beta*dw + sum over output pixels of dy * x(tap). */
int cfp_dwconv3x3_dgrad(const void* dy, int dy_ld, const void* w, void* dx, int dx_ld, int B, int H, int W, int C, int stride,
                        int pad_t, int pad_l, int Ho, int Wo, int accumulate, int dtype, cfp_stream_t stream);
size_t cfp_dwconv3x3_wgrad_ws_bytes(int C);
int cfp_dwconv3x3_wgrad(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, int B, int H, int W, int C, int stride,
                        int pad_t, int pad_l, int Ho, int Wo, float beta, int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* out[i] = idx[i] >= 0 ? x[idx[i]] : 0 (+= when accumulate), idx int32 on the device: crop / regroup / window partition /
 * inside-outside partition of token rows (fusion.py:132-157, transformer.py:101-116,215-234); the maps are injective, so
 * the adjoint of a gather is the gather with the inverse map. */
int cfp_index_rows(const void* x, int x_ld, const int* idx, void* out, int out_ld, long long n_out, int C, int accumulate, int dtype,
                   cfp_stream_t stream);
/* Backward of the full-map bilinear resize (align_corners=True) [B,Hs,Ws,C] -> [B,Hd,Wd,C]: dx (+= when accumulate). */
int cfp_resize_bilinear_bwd(const void* dy, int dy_ld, void* dx, int dx_ld, int B, int Hs, int Ws, int Hd, int Wd, int C,
                            int accumulate, int dtype, cfp_stream_t stream);
/* Adaptive bins (deltar.py:53-59): edges = cumsum(pad((max-min)*w, min)), centres = mid-points; and the adjoint. */
int cfp_bin_centers(const float* widths_normed, float min_val, float max_val, float* edges, float* centers, int B, int NB,
                    cfp_stream_t stream);
int cfp_bin_centers_bwd(const float* dcenters, float min_val, float max_val, float* dwidths_normed, int B, int NB, cfp_stream_t stream);
/* pred = sum_n softmax(logits)[n] * centres[b][n] (deltar.py:51,61) with logits [B*HW, NB] rows; with dpred != NULL the
 * backward instead: dlogits and dcentres (pred unused).  ws: cfp_softmax_expect_ws_bytes (backward only). */
size_t cfp_softmax_expect_ws_bytes(int B, int HW, int NB);
int cfp_softmax_expect(const void* logits, int ld, const float* centers, float* pred, const float* dpred, void* dlogits, int dl_ld,
                       float* dcenters, int B, int HW, int NB, int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Linear attention, training form (attention.py:20-52 and its autograd) on contiguously grouped tokens:
 * q [N*L, heads*d], k, v [N*S, heads*d] -> out [N*L, heads*d]; `state` (cfp_linattn_state_bytes) keeps KV and Ksum of
 * every (group, head) for the backward call, which returns dq, dk, dv.  d in {4, 8, 16, 32}.
 * ws (cfp_linattn_ws_bytes, may be 0 / NULL): with fewer than 512 (group, head) pairs -- the global attentions, N = batch --
 * the token axes are split over more workgroups and the partial [d x (d+1)] states meet in ws, added in a fixed order;
 * without ws one workgroup per (group, head) walks all tokens (same values up to float32 summation order). */
size_t cfp_linattn_state_bytes(int N, int heads, int d);
size_t cfp_linattn_ws_bytes(int N, int L, int S, int heads, int d);
int cfp_linattn_fwd(const void* q, int q_ld, const void* k, int k_ld, const void* v, int v_ld, void* out, int out_ld, float* state,
                    int N, int L, int S, int heads, int d, float eps, int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);
int cfp_linattn_bwd(const void* q, int q_ld, const void* k, int k_ld, const void* v, int v_ld, const void* dout, int do_ld,
                    const float* state, void* dq, int dq_ld, void* dk, int dk_ld, void* dv, int dv_ld, int N, int L, int S,
                    int heads, int d, float eps, int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);
/* cfp_linattn_fwd / _bwd with the live key count read from DEVICE memory (`s_dev`, the n_inside field of a zone record):
 * S stays the row pitch of k / v (the capacity of the inside buffer), rows >= *s_dev are left out of KV and Ksum, the
 * v / S ... * S pair uses *s_dev, and their dk / dv rows are written as zeros (transformer.py:215-234 with the zone rectangle
 * of a dynamic-geometry training step: the DAPM keys are the inside tokens, whose count changes between replays). */
int cfp_linattn_fwd_dev(const void* q, int q_ld, const void* k, int k_ld, const void* v, int v_ld, void* out, int out_ld, float* state,
                        int N, int L, int S, int heads, int d, float eps, int dtype, void* ws, size_t ws_bytes, const int* s_dev,
                        cfp_stream_t stream);
int cfp_linattn_bwd_dev(const void* q, int q_ld, const void* k, int k_ld, const void* v, int v_ld, const void* dout, int do_ld,
                        const float* state, void* dq, int dq_ld, void* dk, int dk_ld, void* dv, int dv_ld, int N, int L, int S,
                        int heads, int d, float eps, int dtype, void* ws, size_t ws_bytes, const int* s_dev, cfp_stream_t stream);

/* Dynamic zone geometry of the training step (csrc/zone_window.hip).  `rec` is an int32[9] DEVICE record
 * (geometry.zone_record): sy, sx, tzh, tzw (the batch zone rectangle in token coordinates, fusion.py:70-84), y0, y1, x0, x1
 * (its part inside the H x W map, fusion.py:104), n_inside; it may change between replays of a captured step.  Token maps
 * are [B*H*W, C] rows, zone tokens [(B*zn*zn)*(p1*p2), C] (grid Gh x Gw = zn*p1 x zn*p2).  Backwards are gather-form
 * (deterministic, no atomics).  f32 / bf16 / f16, C a multiple of the 16-byte vector.
 * cfp_zone_crop      -- fusion.py:129-133: F.pad + crop [sy:sy+tzh, sx:sx+tzw], bilinear (align_corners) resize to Gh x Gw
 *                       when the extent differs, rearrange into zones; extent == grid: an exact copy.
 * cfp_zone_crop_bwd  -- its adjoint into a full [B*H*W, C] map (zero outside the rectangle).
 * cfp_zone_paste     -- fusion.py:136-157: out = tok + resize(zone grid -> tzh x tzw) on the clipped rectangle, tok elsewhere
 *                       (no_skip_inside: the caller zeroes the rectangle of tok first, cfp_zone_rect_rows mode 0).
 * cfp_zone_paste_bwd -- dz of the pasted term (dtok is the incoming gradient itself).
 * cfp_zone_rect_rows -- transformer.py:215-234 / fusion.py:156: mode 0 out = x with the rectangle's rows zeroed [B*H*W];
 *                       mode 1 out [B*cap] = the rectangle's rows per image, row-major, rows >= n_inside zero; mode 2 the
 *                       adjoint of mode 1 (x [B*cap] -> out [B*H*W], zero outside the rectangle). */
int cfp_zone_crop(const void* tok, int tok_ld, const int* rec, void* out, int out_ld, int B, int H, int W, int C, int zn, int p1, int p2,
                  int dtype, cfp_stream_t stream);
int cfp_zone_crop_bwd(const void* dz, int dz_ld, const int* rec, void* dtok, int dtok_ld, int B, int H, int W, int C, int zn, int p1, int p2,
                      int dtype, cfp_stream_t stream);
int cfp_zone_paste(const void* tok, int tok_ld, const void* z, int z_ld, const int* rec, void* out, int out_ld, int B, int H, int W, int C,
                   int zn, int p1, int p2, int dtype, cfp_stream_t stream);
int cfp_zone_paste_bwd(const void* dy, int dy_ld, const int* rec, void* dz, int dz_ld, int B, int H, int W, int C, int zn, int p1, int p2,
                       int dtype, cfp_stream_t stream);
int cfp_zone_rect_rows(const void* x, int x_ld, const int* rec, void* out, int out_ld, int B, int H, int W, int C, int cap, int mode,
                       int dtype, cfp_stream_t stream);

/* Weight gradient of the large-kernel depthwise convolution of LKPM (convnext.py:30, k = 7/15/31, zero padding (k-1)/2):
 * dw[C][k][k] f32 = beta*dw + sum over pixels of dy * x(tap).  The data gradient is cfp_dwconv_large_nhwc with the kernel
 * flipped in both axes. */
size_t cfp_dwconv_large_wgrad_ws_bytes(int B, int H, int W, int C, int k);
int cfp_dwconv_large_wgrad(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, int B, int H, int W, int C, int k, float beta,
                           int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream);

/* Bin-width normalisation out = x / sum_c x over f32 rows (decoder.py:36); with dy != NULL its backward
 * out = (dy - sum_c(dy * y)) / s instead (x = the forward input). */
int cfp_row_normalize(const float* x, const float* dy, float* out, int rows, int C, cfp_stream_t stream);

/* cfp_add_rowtable / cfp_rowtable_grad with the window origin (oy, ox) read from DEVICE memory (int32[2], clamped to the
 * Ht x Wt table): the random positional-encoding window of fusion.py:87-91 can change between replays of a captured graph. */
int cfp_add_rowtable_dev(const void* in, int in_ld, const float* table, void* out, int out_ld, int rows, int C, int H, int W,
                         int Ht, int Wt, const int* oyox, int dtype, cfp_stream_t stream);
int cfp_rowtable_grad_dev(const void* dx, int ld, float* dtable, int B, int H, int W, int C, int Ht, int Wt, const int* oyox,
                          float beta, int dtype, cfp_stream_t stream);

/* NYU training augmentation in one pass (src/dataloader/nyu.py:128-136,204-245,266-285): crop to H x W at (x0, y0), optional
 * horizontal flip, optional gamma / brightness / per-channel colour gain + clip, /255, ImageNet normalisation; depth
 * millimetres -> metres.  rgb_u8 [B,H0,W0,3] and depth_mm [B,H0,W0] uint16 (may be NULL together with depth_out) on the device;
 * params_i [B,4] int32 = (x0, y0, flip, do_augment), params_f [B,2] f32 = (gamma, brightness), colors [B,3] f64 on the
 * device -- the draws themselves stay on the host like in the reference; mean3 / std3 are HOST arrays of 3 floats.
 * image_out [B,3,H,W] f32, depth_out [B,1,H,W] f32.  Crop origins are clamped to the source image. */
int cfp_nyu_augment(const unsigned char* rgb_u8, const unsigned short* depth_mm, int B, int H0, int W0, const int* params_i,
                    const float* params_f, const double* colors, int H, int W, const float* mean3, const float* std3, float* image_out,
                    float* depth_out, cfp_stream_t stream);

/* The random rotation that precedes it (nyu.py:121-124, 200-202): PIL `Image.rotate(angle, BILINEAR)` on the RGB image and
 * `rotate(angle, NEAREST)` on the 16-bit depth, same size, zero fill, byte-exact with Pillow 12 (float64 arithmetic in
 * Pillow's operation order).  matrices [B,6] f64 on the device = Pillow's destination->source affine matrix per sample
 * (computed on the host from the drawn angle exactly as Image.rotate does, cfpnet_amd/augment.py: rotate_matrix).
 * rgb_u8 / rgb_out [B,H,W,3] uint8, depth_mm / depth_out [B,H,W] uint16; either pair may be NULL.  Not in place. */
int cfp_nyu_rotate(const unsigned char* rgb_u8, const unsigned short* depth_mm, unsigned char* rgb_out, unsigned short* depth_out,
                   int B, int H, int W, const double* matrices, cfp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CFPNET_HIP_H */
