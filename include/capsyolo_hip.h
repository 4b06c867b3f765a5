/* capsyolo_hip.h -- C-ABI of libcapsyolo_hip.so (hand-written gfx950 kernels).
 *
 * Drop-in boundary for the training hot path of
 * Cranial-XIX/cs231-capsule-yolo-traffic-sign-detection.  The reference has no FFI
 * (all arithmetic is torch ATen calls); each entry point below replaces the ATen
 * work issued by the cited reference lines.  Conventions for EVERY function:
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller
 *     (the PyTorch caching allocator), valid on `stream`; nothing is allocated,
 *     freed or retained by the library;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous;
 *   - re-entrant, no mutable global state (forward is called from the Python
 *     main thread, backward from the autograd engine thread);
 *   - returns 0 on success, otherwise a non-zero code (hipError_t for runtime
 *     errors, CY_EINVAL for rejected arguments); capsyolo_last_error() gives
 *     the text for the calling thread.
 * Activations are NHWC fp32 unless a stride set says otherwise.
 */
#ifndef CAPSYOLO_HIP_H
#define CAPSYOLO_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define CY_EINVAL 10001

const char* capsyolo_last_error(void);
int capsyolo_abi_version(void);

/* ------------------------------------------------------------------ convolution as implicit GEMM
 * Replaces nn.Conv2d forward / input-gradient / weight-gradient:
 * models.py:90 (conv1), 60-62 (primary capsule convs), 98-110 (decoder convs),
 * 132-223 (DarkNet), 347-363 (DarkCapsuleNet backbone).
 *
 * One description drives forward and input-gradient: a "virtual output grid"
 * [B,Ho,Wo] of pixels, each the sum over TH x TW taps of a Cin-vector of X times
 * a [Cin x N] weight slice:
 *   iy = oy*in_stride + dy0 + a*dstep,  ix = ox*in_stride + dx0 + b*dstep   (zero outside X)
 *   Y[b, oy*out_stride+out_oy, ox*out_stride+out_ox, n] = act(sum + bias[n])
 * X is addressed through element strides (xs_*), so NCHW inputs work (Cin%32 != 0 path).
 */
typedef struct {
  const float* X; const float* Wp; float* Y; const float* bias; double* stats;
  long long xs_b, xs_y, xs_x, xs_c;
  int B, Hi, Wi, Cin;
  int Ho, Wo, N;
  int TH, TW, in_stride, dy0, dx0, dstep;
  int Hy, Wy, out_stride, out_oy, out_ox;
  int act;            /* 0 none, 1 ReLU, 2 LeakyReLU with slope act_slope (last field) */
  /* Optional (input-gradient launches): Y is the gradient with respect to lrelu(bn_z * bn_scale + bn_shift), the
   * activated output of the PRODUCER block whose raw convolution output bn_z has Y's layout.  The epilogue then also
   * accumulates that BatchNorm's backward sums over the pixels it stores -- per channel n:
   *   d = Y * (bn_z*scale+shift > 0 ? 1 : bn_slope),  bn_red[copy][n][0] += d,  bn_red[copy][n][1] += d * (bn_z - mean) * invstd
   * (bn_red[CY_STATS_COPIES][N][2] doubles, zeroed by the caller) -- which replaces the cy_bn_bwd_reduce pass
   * (loss_fns / autograd of models.py:349-351).  All NULL / 0 when unused.
   * cy_conv_gemm_bf16 (bf16 output only): bn_z points to bf16 values, and the kernel STORES d (the premasked gradient, rounded to
   * bf16) and sums the stored values: the producer's cy_bn_bwd_apply_bf16 then runs with slope 1. */
  const float* bn_z; const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_invstd;
  double* bn_red;
  float bn_slope;
  float act_slope;    /* act == 2: Y = max(v, act_slope * v), 0 <= act_slope <= 1 -- the eval-mode forward of a conv -> BatchNorm ->
                       * LeakyReLU block whose BatchNorm was folded into weights and bias (cy_bn_fold_eval) */
  /* Optional workspace of cy_conv_gemm (fp32): ws_floats >= cy_conv_gemm_ws_floats(a) floats, 16-byte aligned.  A layer whose
   * output grid is far below the chip (CapsuleNet's primary-capsule convolution, models.py:60-62: 42 tiles, K = 20736) then runs
   * several blocks per tile on shares of the reduction; the shares' partial sums are added in a fixed order (deterministic).
   * NULL / 0: never split. */
  float* ws; long long ws_floats;
} cy_conv_gemm_t;

/* First layer of the backbones (models.py:347-349 DarkCapsuleNet conv_1 3 -> 128, models.py:132-136 DarkNet conv_1
 * 3 -> 32): 3x3 / stride 1 / pad 1 on the NCHW image X[B][3][H][W] (W % 32 == 0) with PyTorch-layout weights
 * W[Cout][3][3][3], Cout in {32, 64, 128}; Y[B][H][W][Cout] NHWC.  bias / stats as in cy_conv_gemm (either may be NULL).
 * Y may be NULL when stats is given (statistics only: the block's backward recomputes z, cy_conv1_bn_bwd_*).
 * Optional scale / shift [Cout] and slope (then stats must be NULL): Y = lrelu((conv + bias) * scale + shift), the second
 * pass of a conv -> BatchNorm -> LeakyReLU block -- recomputing this layer is cheaper than reading its output back.
 * A store-bound layer: persistent waves, operands from registers / L2, no LDS. */
int cy_conv1_3x3_fwd(const float* X, const float* W, const float* bias, float* Y, double* stats, const float* scale,
                     const float* shift, float slope, int B, int H, int Wd, int Cout, void* stream);
/* The statistics of that layer's output WITHOUT computing it: stats[co] += (sum z, sum z^2) over all pixels from the 28 x 28
 * moment matrix of the 27-element input patches (one Gram-matrix pass over the image, MFMA with both operands the same
 * register), the weights and the bias -- replaces the statistics-only call of cy_conv1_3x3_fwd for any Cout.  W % 32 == 0;
 * ws: cy_conv1_3x3_stats_ws_floats(B, H) floats (partial matrices; 8-byte aligned). */
long long cy_conv1_3x3_stats_ws_floats(int B, int H);
long long cy_conv1_3x3_stats_m2_offset(int B, int H);   /* float offset of the double M2[32][32] inside ws after the call */
int cy_conv1_3x3_stats(const float* X, const float* W, const float* bias, double* stats, float* ws, int B, int H, int Wd,
                       int Cout, void* stream);
/* ... and its weight gradient dW[Cout][3][3][3] from X and dZ[B][H][W][Cout] (the weight-gradient half of nn.Conv2d
 * backward for that layer); ws: cy_conv1_3x3_wgrad_ws_floats floats (one partial slab per persistent wave, added up in a
 * fixed order: deterministic). */
long long cy_conv1_3x3_wgrad_ws_floats(int B, int H, int Wd, int Cout);
int cy_conv1_3x3_wgrad(const float* X, const float* dZ, float* dW, float* ws, int B, int H, int Wd, int Cout, void* stream);
/* Backward of that layer's whole conv -> BatchNorm -> LeakyReLU block from dA, the gradient with respect to the activation
 * (nn.Conv2d / nn.BatchNorm2d / nn.LeakyReLU backward, models.py:347-348), without z and dz in memory: both passes
 * recompute z = conv(X) + bias tile by tile.  Pass 1: red[CY_STATS_COPIES][Cout][2] (zeroed by the caller) += (sum d,
 * sum d xhat) like cy_bn_bwd_reduce.  Pass 2: with red[Cout][2] summed over the copies (and ranks) and count = pixels per
 * channel of the (global) batch, dW[Cout][3][3][3] = weight gradient of dz = scale (d - red0/count - xhat red1/count);
 * dgamma = red1, dbeta = red0 as in cy_bn_bwd_apply.  ws: cy_conv1_bn_bwd_wgrad_ws_floats floats. */
int cy_conv1_bn_bwd_reduce(const float* X, const float* W, const float* bias, const float* dA, const float* scale,
                           const float* shift, const float* mean, const float* invstd, float slope, double* red, int B, int H,
                           int Wd, int Cout, void* stream);
long long cy_conv1_bn_bwd_wgrad_ws_floats(int B, int H, int Wd, int Cout);
int cy_conv1_bn_bwd_wgrad(const float* X, const float* W, const float* bias, const float* dA, const float* scale,
                          const float* shift, const float* mean, const float* invstd, float slope, const double* red,
                          long long count, float* dW, float* ws, int B, int H, int Wd, int Cout, void* stream);
/* The same three passes at the boundary to the bf16 path ("precision": "bf16", BASELINE configs[4]; models.py:347-351): the
 * first block's activation leaves as bf16 NHWC (Y) and its backward takes the second block's bf16 input gradient (dA) --
 * no fp32 copy of the activation or of its gradient exists.  Everything else as in the fp32 entry points above. */
int cy_conv1_3x3_fwd_act_bf16(const float* X, const float* W, const float* bias, void* Y, const float* scale,
                              const float* shift, float slope, int B, int H, int Wd, int Cout, void* stream);
int cy_conv1_bn_bwd_reduce_bf16(const float* X, const float* W, const float* bias, const void* dA, const float* scale,
                                const float* shift, const float* mean, const float* invstd, float slope, double* red, int B,
                                int H, int Wd, int Cout, void* stream);
int cy_conv1_bn_bwd_wgrad_bf16(const float* X, const float* W, const float* bias, const void* dA, const float* scale,
                               const float* shift, const float* mean, const float* invstd, float slope, const double* red,
                               long long count, float* dW, float* ws, int B, int H, int Wd, int Cout, void* stream);
/* The same backward in ONE pass over dA (instead of cy_conv1_bn_bwd_reduce + cy_conv1_bn_bwd_wgrad) for a block whose forward
 * statistics came from cy_conv1_3x3_stats: the pass sums d = dA * lrelu'(y) and the weight gradient OF d; since the layer is
 * linear in its input patches, sum d*xhat and the weight gradient of dz follow from those and the forward's patch moments M2
 * (ws + cy_conv1_3x3_stats_m2_offset of that call) in closed form.  redc: [CY_STATS_COPIES][Cout][2] doubles, zeroed by the
 * caller; dW[Cout][27], dgamma, dbeta [Cout] written; red_out (optional) [Cout][2] = (sum d, sum d*xhat);
 * ws: cy_conv1_bn_bwd_wgrad_ws_floats floats. */
int cy_conv1_bn_bwd_onepass(const float* X, const float* W, const float* bias, const float* dA, const float* scale,
                            const float* shift, const float* mean, const float* invstd, float slope, const double* M2,
                            double* redc, float* dW, float* dgamma, float* dbeta, double* red_out, float* ws, int B, int H,
                            int Wd, int Cout, void* stream);
int cy_conv1_bn_bwd_onepass_bf16(const float* X, const float* W, const float* bias, const void* dA, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, float slope, const double* M2,
                                 double* redc, float* dW, float* dgamma, float* dbeta, double* red_out, float* ws, int B, int H,
                                 int Wd, int Cout, void* stream);
/* The fp32 one-pass backward WITHOUT the recomputation of z: that pass needs of z only the sign of y = z * scale + shift, which the
 * activation pass of the forward has in registers.  cy_conv1_3x3_fwd_act_mask is the activation pass of cy_conv1_3x3_fwd (scale /
 * shift mandatory, the same Y to the byte) that also stores one bit per element, y > 0, in mask (cy_conv1_signmask_bytes bytes =
 * B H W Cout / 8; mask NULL: exactly cy_conv1_3x3_fwd's launch); cy_conv1_bn_bwd_onepass_mask is cy_conv1_bn_bwd_onepass reading
 * those bits instead of the image taps and the weights.  Layout: per 32-pixel tile (global tile number) and lane of the wave one
 * word of 16 Cout / 32 bits, mask[tile][lane] -- two 32-bit words for Cout = 128, one for 64, a 16-bit word for 32; the lane's
 * elements e = (Cout / 32) r + nt (accumulator row r, channel tile nt) fill the words from the top bit down.  The bit is y > 0
 * of y = fma(conv + bias, scale, shift), operation for operation what cy_conv1_bn_bwd_onepass recomputes, so the two backward
 * entry points give the same results to the bit.  (The stored activation comes from fma(conv, scale, bias * scale + shift): with
 * a bias, an element whose y lies within rounding of zero can be stored with the other sign than its bit.)  Y, dA and mask
 * 16-byte aligned. */
long long cy_conv1_signmask_bytes(int B, int H, int Wd, int Cout);
int cy_conv1_3x3_fwd_act_mask(const float* X, const float* W, const float* bias, float* Y, const float* scale,
                              const float* shift, float slope, void* mask, int B, int H, int Wd, int Cout, void* stream);
int cy_conv1_bn_bwd_onepass_mask(const float* X, const float* W, const float* bias, const float* dA, const void* mask,
                                 const float* scale, const float* shift, const float* mean, const float* invstd, float slope,
                                 const double* M2, double* redc, float* dW, float* dgamma, float* dbeta, double* red_out,
                                 float* ws, int B, int H, int Wd, int Cout, void* stream);

/* number of floats of a packed-weight buffer for (K = TH*TW*Cin, N) */
long long cy_conv_packed_floats(int K, int N);
/* pack PyTorch-layout weights W[Cout][Cin][KH][KW] for the forward GEMM of a (sub)set of taps:
 * tap (a,b) uses kernel element (kh0 + a*kstep, kw0 + b*kstep);  transpose=1 packs the
 * input-gradient operand (rows = (tap, cout), columns = cin). */
int cy_conv_pack_weights(const float* W, float* Wp, int Cout, int Cin, int KH, int KW,
                         int TH, int TW, int kh0, int kw0, int kstep, int transpose, void* stream);
/* Y = conv(X) (+bias, +act); if stats != NULL also accumulates per-channel sum / sum-of-squares of the
 * pre-activation output into stats[CY_STATS_COPIES][N][2] (double), which the caller zeroed: every block adds into
 * copy (block id mod CY_STATS_COPIES), so that tens of thousands of blocks do not queue on 2 N addresses (conv_1's
 * launch was bound by exactly that); cy_bn_finalize adds the copies up. */
#define CY_STATS_COPIES 16
int cy_conv_gemm(const cy_conv_gemm_t* a, void* stream);
long long cy_conv_gemm_ws_floats(const cy_conv_gemm_t* a);   /* 0: this launch does not split its reduction */

/* weight gradient: dW[Cout][Cin][KH][KW] = sum over pixels of X-patch (x) dZ.
 * slabs: workspace of cy_conv_wgrad_ws_floats() floats.  dZ is NHWC [B,Ho,Wo,N] contiguous. */
typedef struct {
  const float* X; const float* dZ; float* dW; float* slabs;
  long long xs_b, xs_y, xs_x, xs_c;
  int B, Hi, Wi, Cin;
  int Ho, Wo, N;
  int KH, KW, stride, pad;
} cy_conv_wgrad_t;
long long cy_conv_wgrad_ws_floats(const cy_conv_wgrad_t* a);
int cy_conv_wgrad(const cy_conv_wgrad_t* a, void* stream);

/* Fused Winograd F(2x2,3x3) for 3x3 / stride 1 / pad 1 convolutions on NHWC (2.25x fewer multiplies than the
 * implicit GEMM; fp32 error ~1e-6 relative).  U = cy_wino_pack_weights(W[Cout][Cin][3][3]); transpose=1 packs
 * the input-gradient operand (then call with X = dZ, Cin = layer Cout, Cout = layer Cin).  Cin % 8 == 0.
 * bias / stats as in cy_conv_gemm (either may be NULL). */
long long cy_wino_packed_floats(int Cin, int N);
int cy_wino_pack_weights(const float* W, float* U, int Cout, int Cin, int transpose, void* stream);
int cy_conv3x3_winograd(const float* X, const float* U, float* Y, const float* bias, double* stats, float out_slope,
                        int B, int H, int W, int Cin, int Cout, void* stream);
/* The same with an optional workspace: a launch WITHOUT an epilogue (plain = no bias, no statistics, no activation: the input
 * gradients) whose tiles fill at most half of the CUs (DarkNet's 13 x 13 layers, models.py:196-223: 128 tiles) splits its
 * reduction channels over up to 4 blocks per tile; the shares' slabs are added in a fixed order.  ws: cy_wino_split_ws_floats
 * floats (0 = this shape does not split), 16-byte aligned. */
long long cy_wino_split_ws_floats(int B, int H, int W, int Cin, int Cout, int plain);
int cy_conv3x3_winograd_ws(const float* X, const float* U, float* Y, const float* bias, double* stats, float out_slope,
                           int B, int H, int W, int Cin, int Cout, float* ws, long long ws_floats, void* stream);
/* The same convolution through Winograd F(4x4,3x3) (36 multiplies per 4x4 outputs: 1.78x fewer MFMAs than F(2x2,3x3);
 * fp32 error ~2e-6 relative; replaces the same nn.Conv2d forward / input gradient, models.py:349-351).  Same arguments
 * and meaning as the three functions above; U has its own layout (cy_wino4_packed_floats / cy_wino4_pack_weights). */
long long cy_wino4_packed_floats(int Cin, int N);
int cy_wino4_pack_weights(const float* W, float* U, int Cout, int Cin, int transpose, void* stream);
int cy_conv3x3_winograd4(const float* X, const float* U, float* Y, const float* bias, double* stats, float out_slope,
                         int B, int H, int W, int Cin, int Cout, void* stream);
/* Weight gradient of the same layers through Winograd F(3x3,4x4) (36 multiplies per 4x4 tile of dZ and 3x3 taps: 1.78x fewer MFMAs
 * than F(3x3,2x2) below; fp32 error ~6e-6 relative; replaces the weight-gradient half of nn.Conv2d backward, models.py:349-351).
 * Shapes: cy_wino4_wgrad_ok (H % 4 == 0, W % 16 == 0, Cin % 32 == 0, Cout % 64 == 0, each image below 256 MB); ws:
 * cy_wino4_wgrad_ws_floats floats.  _bn: as cy_conv3x3_winograd_wgrad_bn with a PREMASKED gradient (dA is d = dA lrelu'(y)):
 * dz = d scale + (Z - mean) kb + kc is formed on the way in (kb, kc from red / count) and written to dZ for the input-gradient
 * kernel. */
int cy_wino4_wgrad_ok(int B, int H, int W, int Cin, int Cout);
long long cy_wino4_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout);
int cy_conv3x3_winograd4_wgrad(const float* X, const float* dZ, float* dW, float* ws,
                               int B, int H, int W, int Cin, int Cout, void* stream);
int cy_conv3x3_winograd4_wgrad_bn(const float* X, const float* Z, const float* dA, float* dZ, const float* scale,
                                  const float* mean, const float* invstd, const double* red, long long count,
                                  float* dW, float* ws, int B, int H, int W, int Cin, int Cout, void* stream);
/* Weight gradient of the same layers through Winograd F(3x3,2x2): dW[Cout][Cin][3][3] from X[B][H][W][Cin] and
 * dZ[B][H][W][Cout] (replaces the weight-gradient half of nn.Conv2d backward, models.py:132-223 conv_2 class of
 * layers).  Cin % 64 == 0 and Cout % 64 == 0.  ws: cy_wino_wgrad_ws_floats(B, Cin, Cout) floats (Winograd-domain
 * partial sums, one slab per contiguous range of tile groups -- the batch's B * ceil(H/4) * ceil(W/8) groups are dealt to
 * about one block per CU whatever the batch and map size -- reduced in a fixed order: the result is deterministic). */
long long cy_wino_wgrad_ws_floats(int B, int Cin, int Cout);
int cy_conv3x3_winograd_wgrad(const float* X, const float* dZ, float* dW, float* ws,
                              int B, int H, int W, int Cin, int Cout, void* stream);
/* The same weight gradient with the block's BatchNorm + LeakyReLU backward applied on the way in (replaces pass 2 of
 * nn.BatchNorm2d / nn.LeakyReLU backward, models.py:347-351, for conv_2-class layers: 17 GB of elementwise traffic at the
 * headline shape): the kernel reads the raw convolution output Z and dA, the gradient with respect to the activated
 * output, forms dz = scale * (d - mean(d) - xhat * mean(d * xhat)), d = dA * lrelu'(Z * scale + shift), in registers
 * (red = the sums of cy_bn_bwd_reduce over `count` pixels per channel), feeds it to the MFMAs and also writes it to
 * dZ[B][H][W][Cout] for the input-gradient kernel.  dZ must not alias Z or dA.  dgamma / dbeta: cy_bn_param_grad.
 * premasked != 0: dA is already d (cy_conv4x4s2_winograd_dgrad with bn_red set stores the masked gradient). */
int cy_conv3x3_winograd_wgrad_bn(const float* X, const float* Z, const float* dA, float* dZ, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, float slope, int premasked,
                                 const double* red, long long count, float* dW, float* ws,
                                 int B, int H, int W, int Cin, int Cout, void* stream);

/* Fused Winograd F(2x2,2x2) forward for 4x4 / stride 2 / pad 1 convolutions on NHWC (DarkCapsuleNet conv_3..5,
 * models.py:352-363): the layer is a 2x2 stride-1 convolution of the shifted space-to-depth view of its input, which
 * needs 9 instead of 16 multiplies per 2x2 outputs.  X [B][H][W][Cin] (H, W even, Cin % 8 == 0) -> Y [B][H/2][W/2][Cout];
 * U = cy_wino2_pack_weights(W[Cout][Cin][4][4]); bias / stats as in cy_conv_gemm. */
long long cy_wino2_packed_floats(int Cin, int N);
int cy_wino2_pack_weights(const float* W, float* U, int Cout, int Cin, void* stream);
/* in_scale / in_shift [Cin] (both or neither) + in_slope in (0, 1]: the layer's input is lrelu(X * in_scale[c] + in_shift[c])
 * -- the producer's BatchNorm + LeakyReLU (models.py:349-351) applied on the way into LDS, so that the activation tensor
 * of the previous layer is never written to HBM (X is then the previous layer's raw convolution output). */
/* out_slope in [0, 1] (1 = none): Y = lrelu(conv + bias) -- the eval-mode forward with the block's BatchNorm folded into U and
 * bias (cy_bn_fold_eval); then stats and in_scale must be NULL.  cy_conv3x3_winograd takes the same argument. */
int cy_conv4x4s2_winograd(const float* X, const float* U, float* Y, const float* bias, double* stats,
                          const float* in_scale, const float* in_shift, float in_slope, float out_slope,
                          int B, int H, int W, int Cin, int Cout, void* stream);
/* The same forward through Winograd F(4x4,2x2) (25 multiplies per 4x4 outputs: 1.44x fewer MFMAs than F(2x2,2x2); fp32 error ~3e-6
 * relative; same arguments and meaning as cy_conv4x4s2_winograd, own U layout).  Shapes: cy_wino4s2_ok (H, W even, Cin % 8 == 0, each
 * image below 256 MB). */
int cy_wino4s2_ok(int B, int H, int W, int Cin, int Cout);
long long cy_wino4s2_packed_floats(int Cin, int N);
int cy_wino4s2_pack_weights(const float* W, float* U, int Cout, int Cin, void* stream);
int cy_conv4x4s2_winograd4(const float* X, const float* U, float* Y, const float* bias, double* stats,
                           const float* in_scale, const float* in_shift, float in_slope, float out_slope,
                           int B, int H, int W, int Cin, int Cout, void* stream);
/* Input gradient of the same layers through F(4x4,2x2): the arguments of cy_conv4x4s2_winograd_dgrad below (U =
 * cy_wino4s2_pack_dgrad_weights(W[Cout][Cin][4][4]), cy_wino4s2_dgrad_packed_floats(Cin, Cout) floats; bn_* as there: with bn_red
 * the kernel stores dX * lrelu'(z * scale + shift) and adds the producer BatchNorm's backward sums).  H, W, Cin, Cout are the
 * LAYER's (dX is [B][H][W][Cin]); shapes: cy_wino4s2_dgrad_ok (H, W even, Cin % 64 == 0, Cout % 8 == 0). */
int cy_wino4s2_dgrad_ok(int B, int H, int W, int Cin, int Cout);
long long cy_wino4s2_dgrad_packed_floats(int Cin, int Cout);
int cy_wino4s2_pack_dgrad_weights(const float* W, float* U, int Cout, int Cin, void* stream);
int cy_conv4x4s2_winograd4_dgrad(const float* dZ, const float* U, float* dX, const float* bn_z, const float* bn_scale,
                                 const float* bn_shift, const float* bn_mean, const float* bn_invstd, float bn_slope,
                                 double* bn_red, int B, int H, int W, int Cin, int Cout, void* stream);
/* Weight gradient of the same layers through F(2x2,2x2): dW[Cout][Cin][4][4] from X[B][H][W][Cin] and
 * dZ[B][H/2][W/2][Cout].  Cin % 32 == 0, Cout % 64 == 0, H and W even.  ws: cy_wino2_wgrad_ws_floats(B, Cin, Cout) floats
 * (per-image partial sums in the Winograd domain, reduced in a fixed order: deterministic). */
long long cy_wino2_wgrad_ws_floats(int B, int Cin, int Cout);
int cy_conv4x4s2_winograd_wgrad(const float* X, const float* dZ, float* dW, float* ws,
                                const float* in_scale, const float* in_shift, float in_slope,
                                int B, int H, int W, int Cin, int Cout, void* stream);

/* Input gradient of the same layers through F(2x2,2x2): dX[B][H][W][Cin] from dZ[B][H/2][W/2][Cout]
 * (U = cy_wino2_pack_dgrad_weights(W[Cout][Cin][4][4])).  Cin % 64 == 0, Cout % 8 == 0, H and W even.  bn_* as in
 * cy_conv_gemm_t (optional BatchNorm-backward sums of the producer block; bn_red[CY_STATS_COPIES][Cin][2]).  With bn_red set
 * the kernel stores d = dX * lrelu'(bn_z * bn_scale + bn_shift) -- the gradient at the producer's BatchNorm output, which it
 * has in registers for the sums -- instead of dX: the producer's backward then applies no activation mask (slope 1). */
long long cy_wino2_dgrad_packed_floats(int Cin, int Cout);
int cy_wino2_pack_dgrad_weights(const float* W, float* U, int Cout, int Cin, void* stream);
int cy_conv4x4s2_winograd_dgrad(const float* dZ, const float* U, float* dX, const float* bn_z, const float* bn_scale,
                                const float* bn_shift, const float* bn_mean, const float* bn_invstd, float bn_slope,
                                double* bn_red, int B, int H, int W, int Cin, int Cout, void* stream);

/* per-channel sum over pixels: out[N] = sum_p dZ[p][n]  (bias gradient of convs without BatchNorm).  The row splits are added with
 * float atomics: with more than one split two runs may differ in the last bits. */
int cy_channel_sum(const float* dZ, float* out, long long P, int N, void* stream);
/* The same sum with the same row splits in a FIXED order: every split writes its sum to ws[split][n] and a second launch adds the
 * splits (16 interleaved running sums per channel, then a fixed tree).  No memset and no atomics: the same dZ gives the same bits in
 * every run, which a training step that is to repeat to the bit needs.  ws: cy_channel_sum_ws_floats(P, N)
 * floats, not initialised; 0 means one split, where cy_channel_sum is a fixed order already. */
long long cy_channel_sum_ws_floats(long long P, int N);
int cy_channel_sum_ws(const float* dZ, float* out, float* ws, long long ws_floats, long long P, int N, void* stream);

/* ------------------------------------------------------------------ bf16 convolution path (params.json "precision": "bf16")
 * The backbone's 3x3/s1 and 4x4/s2 layers (models.py:350-363) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
 * activations and raw conv outputs are bf16 NHWC tensors (passed as void* / through the float* fields of cy_conv_gemm_t),
 * weights stay fp32 masters and are packed to bf16 per call, BatchNorm statistics stay double.  Cin and N multiples of 64. */
long long cy_conv_bf16_packed_elems(int K, int N);
/* bf16 image [Np][K] of the GEMM B operand (same tap / transpose semantics as cy_conv_pack_weights) */
int cy_conv_bf16_pack_weights(const float* W, void* Wp, int Cout, int Cin, int KH, int KW, int TH, int TW, int kh0, int kw0,
                              int kstep, int transpose, void* stream);
/* forward / per-parity-class input gradient; X, Wp bf16; Y bf16, or fp32 when out_f32 (the consumer is an fp32 kernel) */
int cy_conv_gemm_bf16(const cy_conv_gemm_t* a, int out_f32, void* stream);
/* a[0 .. ncls-1] (ncls <= 4): descriptors that differ only in Wp, dy0, dx0, out_oy, out_ox -- the output-parity classes of a strided
 * input gradient (models.py:352-363 backward) -- in ONE launch: the classes of a pixel tile run on neighbouring blocks at the same
 * time, so X is fetched from HBM once instead of once per class. */
int cy_conv_gemm_bf16_classes(const cy_conv_gemm_t* a, int ncls, int out_f32, void* stream);
/* The plan the two entry points above launch for the same arguments, without a GPU (host arithmetic; pointers are not read):
 * plan5 = {BM, BN, TAPIN (taps inside a channel chunk), ntiles, blocks}.  Returns what the launch would return for the shape
 * (0, or CY_EINVAL with capsyolo_last_error() set). */
int cy_conv_gemm_bf16_plan(const cy_conv_gemm_t* a, int ncls, int out_f32, int* plan5);
/* weight gradient dW[Cout][Cin][KH][KW] (fp32) of a pad-1 3x3/stride-1 or 4x4/stride-2 layer from bf16 X and dZ;
 * ws: cy_conv_wgrad_bf16_ws_floats() floats of per-split partial sums, added in a fixed order (-1: unsupported shape) */
long long cy_conv_wgrad_bf16_ws_floats(int B, int Ho, int Wo, int Cin, int Cout, int KH, int stride);
int cy_conv_wgrad_bf16(const void* X, const void* dZ, float* dW, float* ws, int B, int Hi, int Wi, int Cin, int Ho, int Wo,
                       int Cout, int KH, int stride, void* stream);
/* ... with the block's BatchNorm backward (pass 2) on the way in (models.py:350-365 backward, "precision": "bf16"): D = the PREMASKED
 * gradient dA * lrelu'(y) (bf16: what the consumer's fused input-gradient epilogue stored), Z = the block's raw convolution output;
 * dz = scale (d - m1 - xhat m2) is written to dZ (bf16, for the input-gradient kernel; bit-identical to cy_bn_bwd_apply_bf16 with
 * slope 1; must not alias D or Z), dW = its weight gradient, dgamma / dbeta (optional) from the sums red[N][2].
 * ws: cy_conv_wgrad_bf16_bn_ws_floats() floats. */
long long cy_conv_wgrad_bf16_bn_ws_floats(int B, int Ho, int Wo, int Cin, int Cout, int KH, int stride);
int cy_conv_wgrad_bf16_bn(const void* X, const void* D, const void* Z, void* dZ, float* dW, float* ws, const float* scale,
                          const float* mean, const float* invstd, const double* red, float* dgamma, float* dbeta, int B, int Hi,
                          int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int stride, void* stream);
/* BatchNorm apply + LeakyReLU and the two backward passes on bf16 tensors (N divides 2048); dA may be fp32 (da_f32) */
int cy_affine_act_bf16(const void* Z, void* A, const float* scale, const float* shift, float slope, long long P, int N,
                       int out_f32, void* stream);
int cy_bn_bwd_reduce_bf16(const void* Z, const void* dA, int da_f32, const float* scale, const float* shift, const float* mean,
                          const float* invstd, float slope, double* red, long long P, int N, void* stream);
int cy_bn_bwd_apply_bf16(const void* Z, const void* dA, int da_f32, void* dZ, const float* scale, const float* shift,
                         const float* mean, const float* invstd, float slope, const double* red, float* dgamma, float* dbeta,
                         long long P, int N, void* stream);
int cy_cast_f32_bf16(const float* in, void* out, long long n, void* stream);
int cy_cast_bf16_f32(const void* in, float* out, long long n, void* stream);

/* ------------------------------------------------------------------ BatchNorm2d (+LeakyReLU), NHWC
 * Replaces nn.BatchNorm2d + nn.LeakyReLU in training and eval mode (models.py:132-223, 347-365). */
/* stats[CY_STATS_COPIES][N][2] (sum, sumsq from cy_conv_gemm / cy_conv3x3_winograd) -> scale/shift (gamma*invstd, beta-mean*scale),
 * mean, invstd; updates running_mean/var with `momentum` (unbiased variance), as torch does. */
int cy_bn_finalize(const double* stats, long long count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps,
                   float* scale, float* shift, float* mean, float* invstd, int N, long long* num_batches_tracked, void* stream);
/* Folds striped double sums: red_out[c][k] = scale * sum_copies red_copies[copy][c][k] (k = 0, 1); dbeta / dgamma
 * (optional) receive the two columns as floats.  Replaces the host-side copy reduction of the BatchNorm backward. */
int cy_bn_red_fold(const double* red_copies, int copies, double scale, double* red_out, float* dgamma, float* dbeta,
                   int N, void* stream);
/* eval mode: scale/shift from the running statistics */
int cy_bn_eval_scale_shift(const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, float* scale, float* shift, int N, void* stream);
/* eval mode: the BatchNorm FOLDED into the convolution in front of it (the eval forward of predict_fns.py:38-43, 65-69 over
 * models.py:132-223, 347-365): Wf[co][...] = W[co][...] * s[co], bf[co] = (bias[co] - running_mean[co]) * s[co] + beta[co] with
 * s = gamma / sqrt(running_var + eps); W is any [Cout][per_out] weight tensor (PyTorch layout), bias may be NULL.  The block's
 * eval forward is then ONE launch: the conv kernel on (Wf, bf) with its LeakyReLU epilogue (out_slope / act = 2). */
int cy_bn_fold_eval(const float* W, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, float eps, float* Wf, float* bf, int Cout, int per_out, void* stream);
/* A = lrelu(Z*scale + shift), negative slope `slope` (1.0 = identity, 0.0 = ReLU); scale/shift may be NULL */
int cy_affine_act(const float* Z, float* A, const float* scale, const float* shift, float slope,
                  long long P, int N, void* stream);
/* backward, pass 1: red[N][2] += (sum dYhat, sum dYhat*xhat), dYhat = dA * lrelu'(Z*scale+shift) */
int cy_bn_bwd_reduce(const float* Z, const float* dA, const float* scale, const float* shift,
                     const float* mean, const float* invstd, float slope, double* red,
                     long long P, int N, void* stream);
/* backward, pass 2: dZ = gamma*invstd*(dYhat - mean(dYhat) - xhat*mean(dYhat*xhat)); dgamma, dbeta written */
int cy_bn_bwd_apply(const float* Z, const float* dA, float* dZ, const float* scale, const float* shift,
                    const float* mean, const float* invstd, const float* gamma, float slope,
                    const double* red, float* dgamma, float* dbeta, long long P, int N, void* stream);
/* dgamma = red[n][1], dbeta = red[n][0] alone (for callers that fuse pass 2 into another kernel) */
int cy_bn_param_grad(const double* red, float* dgamma, float* dbeta, int N, void* stream);
/* activation-only backward: dZ = dA * act'(Z)  (ReLU convs without BN) */
int cy_act_bwd(const float* Z, const float* dA, float* dZ, float slope, long long n, void* stream);

/* ------------------------------------------------------------------ capsule routing
 * Replaces CapsuleLayer.forward, routing branch (models.py:70-79), all n_iter iterations in one
 * launch, and its autograd backward.  u rows are either contiguous [R][N*Din] (gather_g == 0) or
 * read straight from the NHWC feature map [B][4g][4g][256] through the DarkCapsuleNet "cell
 * gather" (models.py:393-398; row = k*B + b).  W is route_weights [N][C][Din][Dout].
 * v_out [R][C][Dout] in row order, or, with the cell gather, [B][g*g][C][Dout] (the layout that
 * view(g,g,B,.).permute(2,0,1,3), models.py:399, presents); dv of the backward uses the same
 * layout.  s_hist [n_iter][R][C][Dout] keeps every iteration's pre-squash sums for the backward. */
typedef struct {
  const float* u; const float* W; float* v_out; float* s_hist;
  int R, N, C, Din, Dout, n_iter;
  int gather_g, gather_B;
  float* ws;            /* workspace of cy_routing_fwd_ws_floats() floats (0 for most shapes: may then be NULL) */
} cy_routing_fwd_t;
/* Few rows (R < ~1000) cannot fill the chip row-wise: the input capsules are then split over blocks too and each
 * routing iteration becomes one phase launch + one finish launch (needs the workspace). */
long long cy_routing_fwd_ws_floats(const cy_routing_fwd_t* a);
int cy_routing_fwd(const cy_routing_fwd_t* a, void* stream);

typedef struct {
  const float* u; const float* W; const float* s_hist; const float* dv;   /* dv [R][C][Dout] */
  float* du;            /* same addressing as u (contiguous rows or NHWC feature-map gradient) */
  float* dW;            /* [N][C][Din][Dout], overwritten */
  float* ws;            /* workspace, cy_routing_bwd_ws_floats() floats */
  int R, N, C, Din, Dout, n_iter;
  int gather_g, gather_B;
} cy_routing_bwd_t;
long long cy_routing_bwd_ws_floats(const cy_routing_bwd_t* a);
int cy_routing_bwd(const cy_routing_bwd_t* a, void* stream);

/* Built shapes: the specialised kernels take C == 1 with N*Din == 4096, Dout == 5, and Din == 8, Dout in {5, 16, 21, 48},
 * C <= 64.  Every other shape of the envelope Din 1..16, Dout 1..64, C 1..256 (any R, N, n_iter; with the cell gather
 * N == 512, Din == 8) runs on the general kernels (csrc/routing_general.hip): cy_routing_fwd / cy_routing_bwd send them
 * there, and the entry points below call them for any shape of the envelope (A/B runs, cross-checks).  They keep the
 * contracts of the specialised ones: the same s_hist, so a forward on one path feeds a backward on the other; bitwise
 * run-to-run determinism; no allocation or host synchronisation (workspace from the _ws_floats queries).  Outside the
 * envelope they return CY_EINVAL and the _ws_floats queries -1. */
int cy_routing_specialised(const cy_routing_fwd_t* a);    /* 1: cy_routing_fwd / _bwd take the shape on the specialised kernels */
long long cy_routing_general_fwd_ws_floats(const cy_routing_fwd_t* a);
int cy_routing_general_fwd(const cy_routing_fwd_t* a, void* stream);
long long cy_routing_general_bwd_ws_floats(const cy_routing_bwd_t* a);
int cy_routing_general_bwd(const cy_routing_bwd_t* a, void* stream);
/* The plan of one routing call, without a GPU (host arithmetic; only the shape fields of `a` are read): which kernels take it, with
 * which launch numbers, and where every buffer lies in the workspace.  backward: the plan of cy_routing_bwd instead of cy_routing_fwd;
 * force_general: the plan of the cy_routing_general_ entry points.  out[0..6] = {path (0 c1, 1 rows_fused, 2 rows_phased, 3 general,
 * 4 mfma_fused, 5 mfma_phased), blocks along the rows, chunks of input capsules, input capsules per chunk, couplings saved for the
 * du / dW kernel (0 / 1), workspace floats (what the _ws_floats query of the path returns), number of regions}, then per region in
 * workspace order {id (0 ds_all, 1 V / V_all, 2 SA, 3 slabs, 4 tail, 5 W, 6 cdb, 7 du_hat, 8 dW_splits), offset, length} in floats;
 * n: the values out can hold (34 always suffice).  Returns 0, or CY_EINVAL with capsyolo_last_error() set for a shape no path takes. */
int cy_routing_plan(const cy_routing_fwd_t* a, int backward, int force_general, long long* out, int n);

/* squash over the last dim (models.py:64-67), rows of D floats; and its backward */
int cy_squash_fwd(const float* s, float* v, long long rows, int D, void* stream);
int cy_squash_bwd(const float* s, const float* dv, float* ds, long long rows, int D, void* stream);
/* capsule length (x**2).sum(-1)**0.5 (models.py:117) and backward */
int cy_length_fwd(const float* v, float* len, long long rows, int D, void* stream);
int cy_length_bwd(const float* v, const float* len, const float* dlen, float* dv, long long rows, int D, void* stream);

/* ------------------------------------------------------------------ losses (forward value + input gradient in one launch)
 * loss_out: one float, overwritten.  Gradients are d(loss)/d(input) for an upstream gradient of 1. */
/* loss_fns.py:187-204 + utils.py:69-85; caps [B,g,g,5] fp32, y [B,g,g,5+C] fp64 */
int cy_darkcapsule_loss(const float* caps, const double* y, int ystride, float* loss_out, float* dcaps,
                        int B, int cells, void* stream);
/* loss_fns.py:145-160 (darkcapsule2_loss): caps [B,g,g,5+C] fp32, y [B,g,g,5+C] fp64 */
int cy_darkcapsule2_loss(const float* caps, const double* y, float* loss_out, float* dcaps, int B, int cells, int C,
                         void* stream);
/* loss_fns.py:163-184 (darkcapsule3_loss, recon off): caps [B,g,g,C,D] fp32 with D = 5 + 16, y [B,g,g,5+C] fp64 */
int cy_darkcapsule3_loss(const float* caps, const double* y, float* loss_out, float* dcaps, int B, int cells, int C, int D,
                         void* stream);
/* loss_fns.py:11-23 margin part; scores [B,C], labels int64 */
int cy_margin_loss(const float* scores, const long long* y, float* loss_out, float* dscores,
                   int B, int C, void* stream);
/* coef * sum((x-recon)^2) / B added into loss_out (loss_fns.py:19-21); drecon written */
int cy_recon_loss_add(const float* x, const float* recon, float coef_over_B, float* loss_out, float* drecon,
                      long long n, void* stream);
/* loss_fns.py:60-142 (dense form); y_pred [B,g,g,5nb+C] fp32, y_true [B,g,g,5+C] fp64; avg_iou_out one float */
int cy_dark_loss(const float* y_pred, const double* y_true, float* loss_out, float* avg_iou_out, float* dpred,
                 int B, int g, int nb, int C, float l_coord, float l_noobj, float img_size, void* stream);
/* out = in * (*scalar)  (backward of a scalar loss with upstream gradient on the device) */
int cy_scale_by_device_scalar(const float* in, const float* scalar, float* out, long long n, void* stream);

/* ------------------------------------------------------------------ linear layers and softmax cross-entropy (csrc/linear.hip)
 * The nn.Linear pair of ConvNet (models.py:22-43) and cnn_loss (loss_fns.py:6-8).  fp32, row-major, W[N][K] as nn.Linear stores it.
 * Supported: M 1..4096 rows, N 1..1024 outputs, K a multiple of 4 up to 2^20, C 1..1024 classes; anything else is CY_EINVAL (the
 * queries return -1).  Tensors read or written 16 bytes at a time (X, W, dX, dW) must be 16-byte aligned.  No atomics: every
 * entry point repeats bit for bit.
 *
 * cy_linear_fwd: Y[M][N] = act(X[M][K] W[N][K]^T + bias), act 0 none / 1 ReLU, bias may be NULL.  The reduction over K runs in
 * `shares` slices of `slice` elements on separate blocks; with more than one share the partial sums go to ws[shares][M][N] and are
 * added in a fixed order (16 interleaved runs of ascending shares, then the 16 sums in ascending order).  The rule (host arithmetic; 256 CUs are assumed when no device answers):
 *   blocks  = ceil(N / 64) * ceil(M / rows),  rows = 16 (M <= 16), 32 (M <= 32), else 64
 *   shares  = min(ceil(2 CUs / blocks), K / (4 M), ceil(K / 128), 256), at least 1
 *             -- two blocks per CU; the partial sums at most a quarter of W's bytes; one share while K fits one slice of 128
 *   slice   = ceil(K / shares) rounded up to a multiple of 64;  shares = ceil(K / slice)
 * ws: cy_linear_fwd_ws_floats() = shares * M * N floats when shares > 1, else 0 (ws may then be NULL). */
int cy_linear_fwd_shares(int M, int N, int K);
int cy_linear_fwd_slice(int M, int N, int K);
long long cy_linear_fwd_ws_floats(int M, int N, int K);
int cy_linear_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, int act, float* ws,
                  void* stream);
/* dX[M][K] = dY[M][N] W[N][K].  X (optional): the layer's own input, the output of a ReLU; then dX[m][k] = 0 where X[m][k] <= 0 --
 * the backward of the ReLU in front of the layer, applied in the store. */
int cy_linear_dgrad(const float* dY, const float* W, float* dX, const float* X, int M, int N, int K, void* stream);
/* dW[N][K] = dY[M][N]^T X[M][K] and (db not NULL) db[N] = the column sums of dY, rows added in ascending order.  The reduction over
 * M is short: the blocks are slices of K, X and dW are streamed once (N <= 128, M <= 64; otherwise X once per 64 rows of dW). */
int cy_linear_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* stream);
/* loss[0] = mean over the rows of -log softmax(scores[M][C])[y], dscores = its gradient; the row maximum is subtracted before exp.
 * y int64; a label outside 0 .. C-1 reads nothing and contributes no target term. */
int cy_softmax_xent(const float* scores, const long long* y, float* loss, float* dscores, int M, int C, void* stream);

/* ------------------------------------------------------------------ gradient with respect to the image (csrc/image_grad.hip)
 * The input gradient of a first layer: a stride-1 convolution that reads the NCHW image.  dx[B][3][H][W] (NCHW fp32) from
 * dy[B][Ho][Wo][Cout] (NHWC fp32, Ho = H + 2 pad - k + 1) and W[Cout][3][k][k]; the activation's derivative and an eval-mode
 * BatchNorm scale are applied on the loads of dy:
 *   dz[p][co]       = dy[p][co] * (act == NULL ? 1 : (act[p][co] > 0 ? 1 : slope)) * (scale == NULL ? 1 : scale[co])
 *   dx[b][c][y][x]  = sum over co, kh, kw of dz[b][y + pad - kh][x + pad - kw][co] * W[co][c][kh][kw]     (terms off the map are absent)
 * act: the block's own OUTPUT [B][Ho][Wo][Cout] (its sign is the sign of the pre-activation for a slope in [0, 1]; other slopes are
 * refused when act is given).  Supported: Cin == 3, k odd in 1..9, pad 0..k/2, Cout 1..1024, H and W >= k - 2 pad, any B whose tile
 * count stays below 2^31; everything else is CY_EINVAL before a launch, and cy_conv_image_grad_ok answers 0 for the shape.  fp32
 * accumulation, no atomics, no workspace: every element of dx is summed by one thread with co, kh, kw ascending, so a call repeats bit
 * for bit.  Tiles of 16 x 32 image pixels per block; partial tiles and taps off the map are predicated. */
int cy_conv_image_grad_ok(int B, int H, int W, int Cout, int k, int pad);
int cy_conv_image_grad(const float* dy, const float* act, const float* scale, const float* W, float* dx, int B, int H, int Wd,
                       int Cin, int Cout, int k, int pad, float slope, void* stream);

/* ------------------------------------------------------------------ attack step and saliency map (csrc/attack.hip)
 * cy_attack_step: one signed-gradient step of FGSM / PGD, in place on x, n elements, every line one fp32 rounding:
 *   s = (g > 0) - (g < 0)                       (0 for g == 0 and for NaN)
 *   t = x + alpha * s                           (alpha * s is exact)
 *   t = min(max(t, x0 - eps), x0 + eps)         (each bound rounded once)
 *   x = min(max(t, lo), hi)
 * alpha, eps >= 0 and lo <= hi, else CY_EINVAL. */
int cy_attack_step(float* x, const float* x0, const float* g, float alpha, float eps, float lo, float hi, long long n, void* stream);
/* out[b][y][x] (uint8) = floor(m / max_b * 255 + 0.5), m = max over the 3 channels of |g[b][c][y][x]| and max_b the largest m of image
 * b (the quotient, the product and the sum each rounded once to fp32).  NaN counts as 0, infinity as FLT_MAX; an image whose max_b is
 * 0 gives zeros.  One workgroup per image: a workgroup reduction for max_b, then one store pass.  No atomics. */
int cy_grad_saliency_u8(const float* g, unsigned char* out, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------ data movement / elementwise around the path
 * Layout permutes standing in for the reference's view/permute/cat glue (models.py:8-19, 80-82):
 * out[b][i1][i2][i3] (contiguous, dims nb x d1 x d2 x d3) = in[b*sb + i1*s1 + i2*s2 + i3*s3];
 * scatter=1 runs the inverse (in is contiguous, out is strided): the backward of the gather. */
/* Device side of the input pipeline: uint8 NHWC [B,H,W,C] -> fp32 (x - 128) / 128, the centring of
 * utils.py:122-123, written NCHW (to_nchw = 1: the layout main.py:57-59 hands to model.forward) or NHWC.  Exact:
 * every value is k / 128.  Lets the host ship 1 byte per sample instead of 4 (GTSRB) or 8 (GTSDB float64). */
int cy_center_u8(const unsigned char* src, float* dst, int B, int H, int W, int C, int to_nchw, void* stream);
int cy_permute4(const float* in, float* out, long long nb, int d1, int d2, int d3, long long sb, long long s1,
                long long s2, long long s3, int scatter, void* stream);
/* nn.MaxPool2d(2) on NHWC (models.py:135-195): x [B,2Ho,2Wo,C] -> y [B,Ho,Wo,C]; idx keeps the argmax (0..3) */
/* conv -> BatchNorm -> LeakyReLU -> MaxPool2d(2) blocks (models.py:135 ... 195) without the full-resolution activation:
 * Y[B][Ho][Wo][C] = max over the 2 x 2 window of lrelu(Z * scale + shift) (Z [B][2 Ho][2 Wo][C], the block's raw convolution output),
 * idx = the winning position 0 .. 3 (first of equals in row-major order, as nn.MaxPool2d); C % 4 == 0.
 * Backward: D[B][2 Ho][2 Wo][C] = [position == idx] dP lrelu'(Z * scale + shift) -- the premasked gradient the block's backward takes
 * (cy_conv3x3_winograd_wgrad_bn premasked = 1 / cy_bn_bwd_apply with slope 1) -- and red[C][2] (doubles, zeroed by the caller) +=
 * (sum D, sum D xhat): the cy_bn_bwd_reduce pass of that block.  C a multiple of 64 (or 4 .. 32). */
int cy_affine_act_maxpool2(const float* Z, const float* scale, const float* shift, float slope, float* Y, unsigned char* idx,
                           int B, int Ho, int Wo, int C, void* stream);
int cy_maxpool2_bwd_bn(const float* dP, const unsigned char* idx, const float* Z, const float* scale, const float* shift,
                       const float* mean, const float* invstd, float slope, float* D, double* red, int B, int Ho, int Wo, int C,
                       void* stream);
int cy_maxpool2_fwd(const float* x, float* y, unsigned char* idx, int B, int Ho, int Wo, int C, void* stream);
int cy_maxpool2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int Ho, int Wo, int C, void* stream);
/* nn.Upsample (nearest, integer factor f; models.py:99-105) on NHWC and its backward */
int cy_upsample_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, int f, void* stream);
int cy_upsample_bwd(const float* dy, float* dx, int B, int Hi, int Wi, int C, int f, void* stream);
int cy_tanh_fwd(const float* x, float* y, long long n, void* stream);
int cy_tanh_bwd(const float* y, const float* dy, float* dx, long long n, void* stream);
/* DarkNet head (models.py:226-236): sigmoid on the first `split` values of each cell, softmax on the other C */
int cy_yolo_head_fwd(const float* x, float* y, long long cells, int split, int C, void* stream);
int cy_yolo_head_bwd(const float* y, const float* dy, float* dx, long long cells, int split, int C, void* stream);
/* Eval / predict side: utils.y_to_boxes_vec (utils.py:288-334 with 233-269) on the device.
 * y [B][g][g][5 nb + C] network output (or ground truth, nb = 1); boxes with confidence > conf_th come out in
 * np.argwhere order: image_idx[n], xy[n][4] = (x1, y1, x2, y2) in pixels (double, the reference's numpy precision),
 * cls[n] (only if C > 0).  image_hw: [B][2] int64 (height, width) per image, or NULL for img_h x img_w everywhere.
 * *count = number of boxes found (may exceed max_boxes: only the first max_boxes are written). */
int cy_yolo_decode_boxes(const float* y, const long long* image_hw, double img_h, double img_w, int B, int g, int nb, int C,
                         float conf_th, int* count, int* image_idx, double* xy, int* cls, int max_boxes, void* stream);
/* Detection metric on the device: metrics.single_img_confusion / calc_iou_individual (metrics.py:99-147) over a
 * batch.  gt / pr: boxes as cy_yolo_decode_boxes returns them (image index ascending, xy[n][4] double).  Adds to
 * out4[0..2] TP (ground-truth boxes overlapped by some prediction with IoU > iou_th), FP (predictions that overlap no
 * ground truth), FN; out4[3] counts malformed boxes (x1 > x2 or y1 > y2; the reference raises AssertionError) and
 * gets +2^20 per image with more than max_per_image boxes.  The caller zeroes out4. */
int cy_detect_confusion(const int* gt_idx, const double* gt_xy, int n_gt, const int* pr_idx, const double* pr_xy, int n_pr,
                        int n_images, double iou_th, int max_per_image, int* out4, void* stream);
/* ------------------------------------------------------------------ two-stage prediction (csrc/predict.hip)
 * predict_fns.dark_class_pred (predict_fns.py:75-82) and metrics.detect_and_recog_mAP (metrics.py:284-339) on the device.
 *
 * Crop + bilinear resize + affine of many boxes in one launch: cv2.resize of whole images (predict_fns.py:38) and of box
 * crops (plot.py:22, predict_fns.py:57).  imgs: packed uint8 HWC images of different sizes (imgs_bytes in all), image k at
 * byte img_off[k] with img_hw[k] = (height, width).  Output b is the half-open rectangle rect[b] = (y0, y1, x0, x1) of image
 * box_img[b], resized as a stand-alone image to OH x OW with the half-pixel convention of INTER_LINEAR
 * (s = (o + 0.5) n_in / n_out - 0.5, neighbours clamped into the crop), interpolated in fp32 and written as
 * (v + shift) * scale to out[n][OH][OW][3], or [n][3][OH][OW] with to_nchw.  cv2's 11-bit fixed-point weights are not
 * reproduced.  A box whose image index or rectangle is out of range is zero-filled and counted in *err (caller-zeroed). */
int cy_crop_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                      const int* box_img, const int* rect, int n, int OH, int OW, float shift, float scale, int to_nchw,
                      float* out, int* err, void* stream);
/* utils.combine_y_hat (utils.py:336-351): y_hat[B][g][g][D + C] = the detector's output dark[B][g][g][D] followed by the class
 * scores[n][C] of the box whose centre lies in the cell (zeros where there is none).  The cell is computed in double in the
 * reference's order (utils.py:198-230) from box_xy[n][4] (pixels of the original image, image_hw[B][2] int64) and the
 * detector's input side; of several boxes in one cell the highest index wins (winner[B g g]: caller-zeroed scratch).
 * A box whose image index, row or column is out of range is counted in *err (caller-zeroed) and ignored. */
int cy_combine_scores(const float* dark, const float* scores, const int* box_img, const double* box_xy, int n,
                      const long long* image_hw, double side, int B, int g, int D, int C, int* winner, float* y_hat, int* err,
                      void* stream);
/* cy_yolo_decode_boxes that also returns conf[n], the stored confidence of every box */
int cy_yolo_decode_boxes_conf(const float* y, const long long* image_hw, double img_h, double img_w, int B, int g, int nb, int C,
                              float conf_th, int* count, int* image_idx, double* xy, int* cls, float* conf, int max_boxes,
                              void* stream);
/* metrics.single_img_confusion for K confidence thresholds x T IoU thresholds in one launch (the sweep of detect_AP and
 * detect_and_recog_mAP).  gt / pr: boxes decoded ONCE at the lowest confidence threshold, with their confidences, sorted by
 * the group key (image, or image * C + class) ascending; one block per group.  A box counts at threshold th iff
 * (double)conf > th, and is hit iff additionally a partner with IoU > iou_t and (double)conf > th exists.  Adds, for every
 * k and t, (TP, FP, FN) to out[k][group % C][t][0..2] (int32, caller-zeroed; C = 1 for the class-agnostic table).
 * *err (caller-zeroed) counts malformed boxes and gets +2^20 per group with more than max_per_group boxes. */
int cy_confusion_sweep(const int* gt_key, const double* gt_xy, const float* gt_conf, int n_gt, const int* pr_key,
                       const double* pr_xy, const float* pr_conf, int n_pr, int n_groups, int C, const double* conf_ths, int K,
                       const double* iou_ths, int T, int max_per_group, int* out, int* err, void* stream);
/* ------------------------------------------------------------------ streaming detector (csrc/serve.hip)
 * The glue of serve.SignDetector: frame -> detector -> crops -> classifier -> labelled boxes with the box list read from device
 * memory, so nothing between the two networks crosses to the host and every launch has a shape that depends on K alone.
 *
 * The rectangle rule of utils.crop_rectangles fused with the crop + resize above, for K slots.  imgs / img_off / img_hw / n_images /
 * imgs_bytes, OH, OW, shift, scale, to_nchw and out are those of the crop + resize entry point; count[1], box_img[K] and
 * box_xy[K][4] = (x1, y1, x2, y2) are what the decode kernel wrote (at least K entries long; *count may exceed K).  Slot s is
 * live iff s < min(*count, K).  A live slot's rectangle is taken in double: the corners truncated towards zero, x clipped to
 * [0, w] and y to [0, h] of image box_img[s], rect_out[s] = (y0, y1, x0, x1) half-open; its pixels are bit for bit those of the
 * crop + resize entry point for that rectangle.  A live slot with a corner that is not finite, an image index outside
 * 0..n_images-1 or an empty rectangle is BAD: zero-filled, rect_out[s] = (0, 0, 0, 0), *err (caller-zeroed) += 1; nothing
 * else happens (one degenerate box must not stop a serving loop).  A dead slot is zero-filled with a zero rectangle and is not
 * counted.  rect_out[K][4] is written for every slot.  K = 0 is valid and launches nothing. */
int cy_boxes_crop_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images,
                            long long imgs_bytes, const int* count, const int* box_img, const double* box_xy, int K, int OH,
                            int OW, float shift, float scale, int to_nchw, float* out, int* rect_out, int* err, void* stream);
/* One record buffer for the host, filled in one launch behind the classifier: `record` (8-byte aligned) holds one
 * cy_detections_header_t followed by K cy_detection_t, 16 + 48 K bytes, little-endian like the device. */
typedef struct {
  int total;        /* boxes over the threshold as the decode kernel counted them (may exceed K) */
  int kept;         /* min(total, K): the records 0..kept-1 are boxes, the others are zeros with cls = -1 */
  int crop_err;     /* bad slots counted by the box crop kernel */
  int resize_err;   /* error word of the whole-frame resize in front of the detector */
} cy_detections_header_t;
typedef struct {
  double xy[4];     /* x1, y1, x2, y2 in pixels of the frame, as decoded */
  int image;        /* frame of the call the box belongs to */
  int cls;          /* arg-max of the slot's class scores: the first maximum wins and a NaN counts as the maximum (np.argmax);
                       -1 for a bad slot (rect = (0, 0, 0, 0)) */
  float conf;       /* the detector's confidence */
  float score;      /* scores[slot][cls]; 0 for a bad slot */
} cy_detection_t;
/* scores[K][C]: the classifier's output for the K crops; count, box_img, box_xy as above, conf[K] from the decode kernel,
 * rect[K][4] = the crop kernel's rect_out; crop_err / resize_err: the two error words (NULL: 0 is recorded). */
int cy_pack_detections(const float* scores, int C, const int* count, const int* box_img, const double* box_xy,
                       const float* conf, const int* rect, const int* crop_err, const int* resize_err, int K, void* record,
                       void* stream);
/* ------------------------------------------------------------------ NV12 frames (csrc/crop_pixel.h, predict.hip, serve.hip, nv12.hip)
 * Cameras and video decode engines deliver NV12: a full-resolution Y plane and a half-resolution plane of interleaved (U, V) pairs,
 * often with a row pitch wider than the frame.  The two crop + resize entry points above exist a second time for such images: the
 * conversion to RGB happens in the tap fetch, so the frame never exists as RGB in memory.
 *
 * Layout.  imgs is one packed buffer of imgs_bytes bytes; image k has its Y plane at byte img_off[k] and
 * img_geom[k] = (H, W, pitch, uv_off), int32 x 4.  The Y sample of pixel (y, x) is the byte at img_off + y pitch + x, its chroma pair
 * (U, V) the two bytes at img_off + uv_off + (y >> 1) pitch + 2 (x >> 1).  Chroma is nearest-neighbour, one pair per 2 x 2 block, and
 * the block is that of the pixel's coordinate in the FRAME, never in a crop.  H, W >= 1 of any parity: the chroma plane has
 * ceil(H / 2) rows of ceil(W / 2) pairs.  An image is valid iff  pitch >= 2 ceil(W / 2),  uv_off >= H pitch,  img_off >= 0  and
 * img_off + uv_off + ceil(H / 2) pitch <= imgs_bytes.  No alignment is assumed: the kernels load bytes.
 *
 * Colour rule.  With the coefficient row below, all in int32, >> the arithmetic shift (floor, not truncation: nearly half of all
 * triples are negative before the clamp in some channel):
 *     y = max(Y - y_off, 0) cy;   u = U - 128;   v = V - 128
 *     R = clamp((y + cvr v         + 2^19) >> 20, 0, 255)
 *     G = clamp((y - cug u - cvg v + 2^19) >> 20, 0, 255)
 *     B = clamp((y + cub u         + 2^19) >> 20, 0, 255)
 * A row is accepted iff 0 <= y_off <= 255 and 255 |cy| + 128 max(|cvr|, |cug| + |cvg|, |cub|) + 2^19 fits int32, so no value before
 * the shift can overflow.  The named rows (capsyolo_amd/nv12.py, MATRICES) are 2^20 fixed point; bt601 = (16, 1220542, 1673527,
 * 409993, 852492, 2116026), e.g. (Y, U, V) = (0, 0, 0) -> (0, 154, 0) and (81, 90, 240) -> (254, 0, 0).
 * The bilinear interpolation then runs in fp32 on those rounded, clamped bytes with the arithmetic of the RGB entry points: every
 * NV12 entry point is bit for bit the RGB entry point on the frame converted by this rule. */
typedef struct { int y_off, cy, cvr, cug, cvg, cub; } cy_yuv_coef_t;
/* cy_crop_resize_u8 on NV12 images: a box whose image index or rectangle is out of range, or whose image is not valid, is
 * zero-filled and counted once in *err. */
int cy_crop_resize_nv12(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images, long long imgs_bytes,
                        cy_yuv_coef_t coef, const int* box_img, const int* rect, int n, int OH, int OW, float shift, float scale,
                        int to_nchw, float* out, int* err, void* stream);
/* cy_boxes_crop_resize_u8 on NV12 images: the same rectangle rule and live / bad / dead slots (a slot of an image that is not valid
 * is bad); K = 0 launches nothing. */
int cy_boxes_crop_resize_nv12(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images,
                              long long imgs_bytes, cy_yuv_coef_t coef, const int* count, const int* box_img, const double* box_xy,
                              int K, int OH, int OW, float shift, float scale, int to_nchw, float* out, int* rect_out, int* err,
                              void* stream);
/* Whole images to packed HWC RGB uint8, image k to out + out_off[k] (H W 3 bytes; the layout cy_draw_boxes_u8 and cy_crop_resize_u8
 * read).  An image that is not valid, or with out_off[k] < 0 or out_off[k] + 3 H W > out_bytes, is left untouched and counted once
 * in *err (caller-zeroed).  At most 65535 images.  For drawing, debugging and tests: the streaming detector does not use it. */
int cy_nv12_to_rgb_u8(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images, long long imgs_bytes,
                      cy_yuv_coef_t coef, unsigned char* out, const long long* out_off, long long out_bytes, int* err, void* stream);
/* ------------------------------------------------------------------ non-maximum suppression (csrc/nms.hip)
 * Greedy confidence-ordered suppression of a decoded box list, per image, with no host synchronisation: two launches whose shapes
 * depend on n_images alone (the list length is read from device memory), so the step captures into a HIP graph.  The reference has
 * no such step; tests/nms_ref.py restates the rule in numpy.
 * Input: the list as cy_yolo_decode_boxes_conf writes it -- count_in[1] (the live length is min(*count_in, n_cap)), box_img[n_cap]
 * ascending, box_xy[n_cap][4] = (x1, y1, x2, y2), conf[n_cap], cls[n_cap] or NULL.
 * Rule: inside an image the boxes are visited by confidence descending, ties to the lower list index (a NaN confidence behind
 * every number).  A box is kept unless an already kept box of its image (class_aware: and of its class) has IoU > iou_th with it,
 * strictly; the IoU is the double-precision one of cy_confusion_sweep (csrc/box_iou.h), and a NaN IoU suppresses nothing.  A
 * malformed box (a corner that is not finite, x1 > x2 or y1 > y2) is kept and suppresses nothing: the crop stage counts it as bad,
 * as without this step.  per_image > 0: only the first per_image survivors of an image stay (0: no cap).
 * Output: keep[n_cap] in list order, 1 or 0 (0 past the live length and for an image index outside 0..n_images-1); the survivors,
 * image ascending and inside an image confidence descending, as copies of their list entries in out_img / out_xy / out_conf /
 * out_cls (written iff cls is given) / out_src (the index in the list), K slots each; *count_out = the survivors (may exceed K:
 * only the first K are written); the slots at and behind min(*count_out, K) are zero-filled.  ws[n_images]: scratch.
 * max_per_image: boxes of one image that fit in LDS (48 bytes each, at most cy_nms_max_per_image() = 3413 in 160 KiB; up to 1024
 * stay inside the 48 KiB a launch gets without opting in).  An image with more live boxes adds 2^20 to *err (caller-zeroed) and
 * all of its boxes get keep = 0.  K = 0 or n_cap = 0 is valid and launches nothing. */
int cy_nms_max_per_image(void);
int cy_nms_boxes(const int* count_in, const int* box_img, const double* box_xy, const float* conf, const int* cls, int n_cap,
                 int n_images, double iou_th, int class_aware, int per_image, int max_per_image, int* keep, int K, int* out_img,
                 double* out_xy, float* out_conf, int* out_cls, int* out_src, int* count_out, int* ws, int* err, void* stream);
/* ------------------------------------------------------------------ tiled detection (csrc/tiles.hip)
 * The detector run on overlapping windows ("tiles") of a frame at close to native scale, and its outputs put back into the frame:
 * cy_yolo_decode_boxes_conf for a batch y[Bt][g][g][5 nb + C] whose images are tiles.  tile_frame[Bt] (ascending), tile_rect[Bt][4] =
 * (y0, y1, x0, x1) half-open and frame_hw[n_frames][2] = (H, W) are the box_img / rect / img_hw tables of the cy_crop_resize_u8 call
 * that cut the tiles.  The reference has no such step; tests/tiles_ref.py restates the rule in numpy.  All in double, not contracted:
 *  1. Tile b is an image of th x tw = (y1 - y0) x (x1 - x0) pixels: a cell's box over conf_th gets its tile-pixel corners
 *     (bx1, by1, bx2, by2) exactly as cy_yolo_decode_boxes_conf computes them with image_hw = (th, tw), the same operations in the
 *     same order.
 *  2. Border rule (skipped when margin < 0).  With (H, W) = frame_hw[tile_frame[b]] the box is dropped, and counted in *dropped
 *     (caller-zeroed, added to), iff  x0 > 0 && bx1 < margin,  or  x1 < W && bx2 > tw - margin,  or  y0 > 0 && by1 < margin,  or
 *     y1 < H && by2 > th - margin.  Only a window edge inside the frame cuts a sign, and a NaN corner drops nothing: a box at such
 *     an edge is left to the neighbouring window that sees it whole, so the windows' overlap has to exceed the largest sign (a
 *     whole-frame view among the tiles serves the signs larger than that).
 *  3. A kept box: xy = (bx1 + (double)x0, by1 + (double)y0, bx2 + (double)x0, by2 + (double)y0), one addition each;
 *     image_idx = tile_frame[b]; conf and cls as cy_yolo_decode_boxes_conf; out_tile (optional, NULL: not written) = b.
 *  4. The kept boxes come out in (tile, row, column, box) order -- frame ascending, what cy_nms_boxes needs -- with no atomic on the
 *     order: identical bits from run to run.  *count = the kept boxes (may exceed max_boxes: only the first max_boxes are written).
 * A tile whose frame index is outside 0..n_frames-1, or whose rectangle is empty or leaves its frame, adds 1 to *err (caller-zeroed)
 * and contributes no box.  Refused before any launch: Bt < 0, g < 1, nb < 1, C < 0, n_frames < 1, max_boxes < 0, a NaN margin, a
 * null pointer (cls only with C > 0).  Bt = 0 or max_boxes = 0 is valid and launches nothing (no word is written).  One workgroup. */
int cy_yolo_decode_tiles_conf(const float* y, const int* tile_frame, const int* tile_rect, const int* frame_hw, int n_frames,
                              double margin, int Bt, int g, int nb, int C, float conf_th, int* count, int* dropped, int* image_idx,
                              double* xy, int* cls, float* conf, int* out_tile, int max_boxes, int* err, void* stream);
/* ------------------------------------------------------------------ sign tracks (csrc/track.hip)
 * The step behind cy_pack_detections in serve.SignDetector: the frame's boxes are joined to the tracks of the frames before, so a
 * sign keeps an id, its class is voted over everything seen so far, and a box seen once is told from a sign.  One launch of one
 * workgroup per frame, no host synchronisation, the tracks live in `state` in device memory: the step captures into a HIP graph.
 * The reference has no such step; tests/track_ref.py restates the rule in numpy.
 * Input: count[1], box_xy[K][4], conf[K], rect[K][4] (the crop kernel's rect_out) and scores[K][C] exactly as cy_pack_detections
 * reads them.  All arithmetic on boxes is double, all arithmetic on class evidence is float, neither is contracted.
 * Rule, per call (= per frame):
 *  1. The live detections are the slots s < min(max(*count, 0), K) whose rect is not all zero (a bad slot, class -1 in the
 *     detections' record, takes no part).  The live tracks are the slots with id != 0.
 *  2. Track t predicts p_t = xy_t + vel_t per corner with motion = 1, xy_t with motion = 0; vel is zero from birth to the first match.
 *  3. A pair (t, s) is a candidate iff box_iou(p_t, det_s) > iou_th, strictly (csrc/box_iou.h, the IoU of cy_nms_boxes and
 *     cy_confusion_sweep, bit for bit); a NaN IoU is no candidate.
 *  4. Greedy assignment: repeatedly the candidate with the largest IoU among those whose track and detection are both still free
 *     is taken; ties go to the lower track slot, then to the lower detection slot.  At most min(K, T) rounds.
 *  5. A matched track takes, in this order: vel = det - xy (the stored box, not the predicted one; kept with motion = 0, where it
 *     is unused); xy = det, conf = conf[s], hits += 1, misses = 0, det = s; evidence[c] = decay * evidence[c] + scores[s][c] for
 *     every class, two rounded float operations.
 *  6. An unmatched live track: misses += 1, det = -1, with motion = 1 xy = xy + vel (it coasts); if then misses > max_misses the
 *     slot is freed (all its fields zero) and counted in deaths.
 *  7. Every unmatched live detection, in slot order, is born into the lowest free slot (slots freed in step 6 of this call are
 *     free): id = ++next_id (ids start at 1 and are never reused), hits = 1, misses = 0, vel = 0, evidence = scores[s], det = s.
 *     With no free slot the detection is counted in dropped and belongs to no track.
 *  8. age += 1 for every live track (a track born in this call ends it with age 1).  cls = the arg-max of evidence under the rule
 *     of cy_pack_detections (the first maximum wins, a NaN counts as the maximum), score = evidence[cls].  A track is confirmed
 *     iff hits >= min_hits.
 *  9. frame += 1.
 * Record (8-byte aligned, 32 + 64 T + 4 K bytes, little-endian like the device): one cy_tracks_header_t, T cy_track_t in slot
 * order (a free slot is all zero), then det_track int[K]: the id of the track detection slot s belongs to after this call, 0 for none.
 * State (8-byte aligned, cy_track_state_bytes(T, C) bytes, 0 for T < 1 or C < 1): opaque; all zero is the valid empty state (no
 * track, frame 0, no id handed out), so a reset is a stream-ordered zero fill (cy_zero_bytes).  The class evidence lives there, in
 * global memory: C is not capped by LDS.
 * Limits, refused before any launch: 1 <= T <= 256; K >= 1; K * T <= cy_track_max_pairs() = 4096 (the candidate table, 8 bytes a
 * pair, stays inside the 48 KiB of LDS a launch gets without opting in); C >= 1; iou_th in [0, 1]; max_misses >= 0; min_hits >= 1;
 * decay in [0, 1]; motion 0 or 1. */
typedef struct {
  int frame;        /* calls since the empty state, this one included */
  int live;         /* tracks with id != 0 after this call */
  int confirmed;    /* of those, tracks with hits >= min_hits */
  int births;       /* tracks born in this call */
  int deaths;       /* tracks freed in this call */
  int dropped;      /* unmatched live detections of this call that found no free slot */
  int next_id;      /* the last id handed out */
  int err;          /* 0 (reserved) */
} cy_tracks_header_t;
typedef struct {
  double xy[4];     /* x1, y1, x2, y2: the last matched detection, or with motion = 1 the box coasted from it */
  int id;           /* 0: a free slot, every field zero */
  int cls;          /* arg-max of the class evidence */
  int age;          /* calls since birth, the one of the birth included */
  int hits;         /* calls with a matched detection, the birth included */
  int misses;       /* calls without one since the last match */
  int det;          /* the detection slot matched or born from in this call, -1 for a live track without one */
  float conf;       /* the detector's confidence of the last matched detection */
  float score;      /* evidence[cls] */
} cy_track_t;
int cy_track_max_pairs(void);
long long cy_track_state_bytes(int max_tracks, int n_classes);
int cy_track_update(const int* count, const double* box_xy, const float* conf, const int* rect, const float* scores, int K, int C,
                    int max_tracks, double iou_th, int max_misses, int min_hits, float decay, int motion, void* state, void* record,
                    void* stream);
/* ------------------------------------------------------------------ box drawing (csrc/draw.hip)
 * plot.draw_boxes (plot.py:24-33) for n boxes in one launch, IN PLACE in a packed buffer of n_images HWC uint8 images described
 * as for cy_crop_resize_u8 (imgs / img_off / img_hw / imgs_bytes); the caller draws into a copy if it still needs the images.
 * Box b belongs to image box_img[b], has the integer corners box_xy[b] = (x1, y1, x2, y2), the 3 bytes box_color[b] in the
 * image's channel order and the label box_label[b] (-1: none, else 0..999; box_label NULL: no box has one).  The result is
 * what drawing the boxes one after the other in index order leaves behind:
 *   outline  cv2.rectangle(img, (x1, y1), (x2, y2), color, 1) taken as: every pixel (x, y) of the image with y in {y1, y2} and
 *            min(x1, x2) <= x <= max(x1, x2), or x in {x1, x2} and min(y1, y2) <= y <= max(y1, y2).  A box partly or wholly
 *            outside the image is clipped (no error); a degenerate or inverted box draws what the rule says.
 *   label    the decimal digits of the label (1-3, most significant first) in the 5 x 7 font glyphs[10][7] (device pointer; one
 *            byte per glyph row, bit 4 = the leftmost column), one empty column between digits, in the box's colour, clipped
 *            at the image border.  The bottom-left corner of the block is (xc, yc) = (floor((x1 + x2) / 2),
 *            floor((y1 + y2) / 2)): rows yc-6 .. yc, digit k in columns xc + 6 k .. xc + 6 k + 4.  (The reference writes the
 *            class NAME with cv2.putText at that origin; neither the names nor the font are available.)
 *   order    where boxes of one image set the same pixel, the highest box index wins.  box_img must ascend (the boxes of an
 *            image contiguous); every pixel is stored by one box only, so the result is bit-identical from run to run.
 * max_items: threads per box, at least 2 * (columns + rows the box spans inside its image) + 119 for a labelled box;
 * 2 * (max width + max height) + 119 always suffices.  *err (caller-zeroed) += the boxes with an image index outside
 * 0..n_images-1, an image outside [0, imgs_bytes), a label outside -1..999, an image index below its predecessor's or more
 * items than max_items; such a box draws nothing.  n = 0 is valid and launches nothing. */
int cy_draw_boxes_u8(unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                     const int* box_img, const int* box_xy, const unsigned char* box_color, const int* box_label, int n,
                     int max_items, const unsigned char* glyphs, int* err, void* stream);
/* ------------------------------------------------------------------ sign-paste augmentation and data-set resize (csrc/augment.hip)
 * build_data.py:80 (a frame resized), 28-29 + 44 (a sign's ROI resized) and 171-288 (signs pasted over a frame, then the frame
 * resized) for n output samples in one launch.  imgs / img_off / img_hw / n_images / imgs_bytes: the background images, and
 * signs / sign_off / sign_hw / n_signs / signs_bytes: the sign images, both packed as for the crop-and-resize entry point above.
 * Sample s reads image sample_img[s], its half-open source rectangle sample_rect[s] = (y0, y1, x0, x1) and the rows
 * begin[s] .. begin[s + 1] - 1 of the paste table (begin has n + 1 entries).  A paste row is 9 ints: (sign, sy0, sy1, sx0, sx1,
 * dy0, dy1, dx0, dx1) = the sign image, its source rectangle, and the destination rectangle in FULL-IMAGE coordinates of the
 * background (both half-open).  Output s is the source rectangle of the composited image resized to OH x OW, the composited image
 * being the background with the sample's pastes applied in table order (a later paste overwrites an earlier one), each paste the
 * sign's source rectangle resized to the destination's size as a stand-alone image.  The composited image is never stored.
 * Both resizes use the half-pixel rule of INTER_LINEAR in exact integers and each yields a BYTE: for output index o of n_out from
 * n_in, num = (2 o + 1) n_in - n_out, r = floor(num / (2 n_out)), a = num - r 2 n_out, taps r and r + 1 clamped into the
 * rectangle (b for the columns), value = ((2 OW - b)(2 OH - a) aa + b (2 OH - a) ab + (2 OW - b) a ba + b a bb + 2 OW OH) /
 * (4 OW OH) rounded down, i.e. round-half-up of the exact bilinear value; equal sizes give the identity.  cv2's 11-bit
 * fixed-point weights are not reproduced.  mode: CY_PASTE_OUT_U8 bytes [n][OH][OW][3]; CY_PASTE_OUT_F32_NHWC and
 * CY_PASTE_OUT_F32_NCHW ([n][3][OH][OW]) hold (byte - 128) / 128 as fp32.  *err (caller-zeroed) += the samples with an image or
 * sign index out of range, an image outside its buffer, a side of 2^24 or more, an empty source rectangle or one that reaches
 * outside its image, an empty destination or one that reaches outside the background, a begin[] that decreases or runs past
 * n_pastes, or more pastes than the query below returns (64); such a sample is zero-filled, the others are untouched.
 * n = 0 is valid and launches nothing; at most 65535 samples per launch; the sign set and the table may be NULL when n_pastes = 0. */
#define CY_PASTE_OUT_U8 0
#define CY_PASTE_OUT_F32_NHWC 1
#define CY_PASTE_OUT_F32_NCHW 2
int cy_paste_resize_max_pastes(void);
int cy_paste_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                       const unsigned char* signs, const long long* sign_off, const int* sign_hw, int n_signs, long long signs_bytes,
                       const int* sample_img, const int* sample_rect, const int* begin, int n, const int* pastes, int n_pastes,
                       int OH, int OW, int mode, void* out, int* err, void* stream);
/* ------------------------------------------------------------------ classifier augmentation (csrc/augment.hip)
 * utils.augmentation (utils.py:126-143) as it is evidently meant, per sample, fused with the gather of a batch from a resident
 * data set, the centring and the NHWC -> NCHW permute.  set [n_set][H][W][3] bytes, labels [n_set]; index [B] sample numbers.
 * shift [n_set][2] = (dy, dx) and light [n_set] = the lightness increase d on the 0..1 V scale are indexed by SAMPLE NUMBER;
 * either may be NULL (no shift / d = 0).  Output pixel (b, y, x) with s = index[b] reads pixel (y - dy, x - dx) of image s; off
 * the image all three channels are exactly 0.0f (grey on the centred scale, not brightened); any int shift is legal.  With the
 * source bytes k as floats and v = max(k): k' = k (v + 256 d) / v for v > 0 and k' = 256 d on all channels for v = 0, which is
 * hsv_to_rgb(rgb_to_hsv(k / 256) + (0, 0, d)); x_out [B][3][H][W] = (k' - 128) / 128, not clipped.  d = 0 gives exactly what
 * cy_center_u8 gives.  y_out [B] = labels[s].  A sample number outside 0..n_set-1 is never dereferenced: its output is zeros,
 * its y_out -1, and *err (caller-zeroed) += 1.  B = 0 is valid and launches nothing; at most 65535 samples per launch. */
int cy_gather_jitter_u8(const unsigned char* set, const long long* labels, int n_set, int H, int W, const int* shift,
                        const float* light, const int* index, int B, float* x_out, long long* y_out, int* err, void* stream);
/* ------------------------------------------------------------------ classifier report (csrc/rank.hip)
 * The integer rank counts behind metrics.recog_auc / recog_pr / recog_acc (metrics.py:9-96; sklearn's roc_curve + auc and
 * average_precision_score there), with no sort of the scores.  scores[N][C] fp32, labels[N] int64; element (i, c) is positive iff
 * c == labels[i], and p_i = scores[i][labels[i]].  Values are compared as floats (-0.0 == +0.0, denormals are not flushed).
 * For every row i, counts[2][N][4] (int32, caller-zeroed) receives (cnt_ge, cnt_gt, tp_ge, tp_gt): the number of elements of
 * a population, and of its positives, whose score is >= p_i and > p_i --
 *   counts[0]: micro, the population is all N*C elements;  counts[1]: per class, the population is column labels[i].
 * *correct (caller-zeroed) += the rows whose label is the FIRST maximum of the row (np.argmax).  *err (caller-zeroed) +=
 * the labels outside 0..C-1 and the non-finite scores (then the counts mean nothing; nothing is read or written out of bounds).
 * order[N] int32: the row indices sorted by label ascending (any order inside a label; the caller sorts the LABELS, the scores
 * are never sorted); an entry outside 0..N-1 or a descending pair of labels is counted in *err.  ws: cy_rank_ws_ints(N, C)
 * ints of scratch.  Integer atomics only: the result is bit-identical from run to run and does not depend on the grid.
 * N*C >= 2^31 is refused (CY_EINVAL); cy_rank_ws_ints returns 0 for such a shape. */
long long cy_rank_ws_ints(int N, int C);
int cy_rank_counts(const float* scores, const long long* labels, const int* order, int N, int C, int* ws, int* counts,
                   int* correct, int* err, void* stream);
/* torch.gather of the labelled capsule (models.py:122): backward=0: out[B][D] = caps[b][y[b]][:];
 * backward=1: caps is d(out) [B][D], out = d(caps) [B][C][D] (zero off the labelled capsule) */
int cy_pick_capsule(const float* caps, const long long* y, float* out, int B, int C, int D, int backward, void* stream);
/* ------------------------------------------------------------------ capsule interpretation (csrc/decoder.hip)
 * The whole decoder forward of CapsuleNet (models.py:96-111) in one launch, with the gather and the perturbation of
 * capsule_interpret.py:58-68 formed in the kernel.  The ten parameter pointers are the state-dict tensors of decoder.0 / 4 / 7 / 10 /
 * 12 as they are (Linear [256][16], convolutions OIHW); nothing is packed on the host.
 * Launch rows: with deltas, row (b, v, i) = (b * 16 + v) * n_delta + i decodes source vector b with deltas[i] added (fp32) to its
 * component v; without, row b decodes source vector b.  Source vector b is caps[b][labels[b]][:] of caps [n][C][16], or, without
 * labels (then C = 1), row b of a dense caps [n][16].  *err (caller-zeroed; required with labels) += the rows whose label lies
 * outside 0..C-1; such rows write nothing.
 * Outputs, each optional, at least one, all from the same arithmetic: out_f32 [rows][3][32][32]; out_u8 [rows][32][32][3] =
 * rint(v * 128 + 128) (half to even) clamped to 0..255; sqerr [rows] = sum over the 3 072 elements of (x[b] - out)^2 against the
 * NCHW image x [n][3][32][32], summed in a fixed order (bit-identical from run to run).  D must be 16.  Nothing is allocated. */
typedef struct {
  const float* caps; const long long* labels; const float* deltas; const float* x;
  const float* lin_w; const float* lin_b; const float* w4; const float* b4; const float* w7; const float* b7;
  const float* w10; const float* b10; const float* w12; const float* b12;
  float* out_f32; unsigned char* out_u8; float* sqerr; int* err;
  int n, C, D, n_delta;
} cy_decoder_t;
int cy_decoder_fwd(const cy_decoder_t* a, void* stream);

/* ------------------------------------------------------------------ optimizer */
/* zero-fill (asynchronous on `stream`) of the per-step scratch arena that the statistics kernels accumulate into */
int cy_zero_bytes(void* p, long long nbytes, void* stream);
/* Gradient bucket of the data-parallel step (between loss.backward() and optimizer.step(), main.py:71-72): every
 * tensor of a list copied into / out of one flat buffer with a scale, ONE launch.  table[k] = {float* tensor,
 * int64 offset into flat, int64 numel}; blockmap[b] = {tensor index, chunk index}. */
int cy_multi_copy(const void* table, const void* blockmap, int n_blocks, int chunk, float* flat, int unpack, float scale,
                  void* stream);

/* torch.optim.Adam step (main.py:72,280) for a list of tensors in ONE launch of n_blocks workgroups, whatever the descriptor selects.
 * table: device array of n_tensors records {param, grad, exp_avg, exp_avg_sq, numel} (5 x 8 bytes); blockmap: device array of
 * n_blocks int2 {tensor index, chunk index}.  The rule, per element, in torch's single-tensor order and in fp32:
 *   g = coef * grad (record != NULL; the gradient tensors are not rewritten) or grad;
 *   m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * g * g;
 *   p -= (lr / bias_corr1) * (m / (sqrt(v) / sqrt(bias_corr2) + eps));
 *   ema += one_minus_decay * (p - ema)  (ema_table != NULL), with the p just stored (= decay * ema + (1 - decay) * p).
 * The three pointers that may be NULL select the variant; each adds to the plain step and changes nothing else of it:
 *   hyper      the scalars come from device memory, {lr, beta1, beta2, eps, bias_corr1, bias_corr2}, with an ema_table two more,
 *              {one_minus_decay, 0}: for a step captured in a HIP graph, whose kernel arguments are frozen (the host refreshes hyper
 *              before every replay, so a captured step follows the step count and a decay schedule).  lr / bias_corr1 and
 *              1 / sqrt(bias_corr2) are then formed on the device, else on the host.  Scalars in device memory cannot be checked
 *              by the entry point: optim.Adam.step_scalars is their only source.
 *   record     cy_grad_clip_finish's record (below): coef = record[1]; record[2] == 0 returns before anything is read or written,
 *              so a skipped step changes no bit of a parameter, exp_avg, exp_avg_sq or average.
 *   ema_table  device array of n_tensors float*, ema_table[k] the moving average of the parameter of table[k] (same numel, fp32, no
 *              overlap with any tensor of table).  one_minus_decay = 1 - decay is formed in double by the caller and rounded ONCE
 *              to fp32, in (0, 1]: the kernel never forms 1.f - decay.  Parameters, exp_avg and exp_avg_sq get the bits of the step
 *              without the average; 36 bytes per element against 28.
 * Refused with a message that names the field: a NULL table or blockmap, n_blocks or chunk <= 0, and with host scalars a bias
 * correction that is not positive or, with an ema_table, a one_minus_decay outside (0, 1]. */
typedef struct {
  const void* table;       /* [n][5] int64 rows (p, g, exp_avg, exp_avg_sq, numel) */
  const void* ema_table;   /* [n] float*; NULL = no moving average */
  const void* blockmap;    /* [n_blocks] (tensor, chunk) */
  const float* hyper;      /* device scalars, 6 floats or 8 with an ema_table; NULL = the host scalars below */
  const float* record;     /* cy_grad_clip_finish's record[4]; NULL = no clipping / guard */
  int n_blocks, chunk;
  float lr, beta1, beta2, eps, bias_corr1, bias_corr2, one_minus_decay;   /* read only when hyper == NULL */
} cy_adam_step_t;
int cy_adam_step(const cy_adam_step_t* a, void* stream);

/* Gradient-norm clipping and the non-finite-step guard of optim.Adam, decided on the device (csrc/gradnorm.hip).  The rule, over
 * every gradient G that one optimizer step applies:
 *   total_norm = sqrt(sum over G of g^2), squares formed and summed in double from the fp32 values, in a fixed order (no atomics:
 *                the same gradients give the same bits);
 *   coef       = min(1, max_norm / (total_norm + 1e-6)) in double, rounded once to fp32; 1 when max_norm <= 0 (no clipping);
 *   go         = 0 when guard != 0 and total_norm is not finite (some gradient element is inf or NaN), else 1.
 * cy_grad_sumsq_multi takes Adam's table and block map (above) and writes partial[b], b < n_blocks, one workgroup per entry; the
 * launches of one step fill consecutive slices of one partial buffer.  Gradients may start at any 4-byte offset.
 * cy_grad_clip_finish adds the n_partial partials in one workgroup and writes record[4] = {total_norm, coef, go, 0}; with go == 0 it
 * also adds 1 to *skipped.  cy_adam_step reads the record. */
int cy_grad_sumsq_multi(const void* table, const void* blockmap, int n_blocks, int chunk, double* partial, void* stream);
int cy_grad_clip_finish(const double* partial, int n_partial, float max_norm /* <= 0: no clipping */, int guard,
                        float* record /* [4] = {total_norm, coef, go (1 | 0), 0} */, long long* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif
