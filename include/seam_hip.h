/*
 * seam_hip.h -- C ABI of libseam_hip.so: the MI355X (gfx950) kernels behind the forward
 * hot path of SEAM Match-RCNN (BASELINE.json north_star).
 *
 * Conventions (every entry point):
 *   - returns int = hipError_t of the launch (0 = success); never throws, never
 *     allocates, never synchronises; asynchronous on `stream` (a hipStream_t, e.g.
 *     torch.cuda.current_stream().cuda_stream passed as void*).
 *   - all pointers are DEVICE pointers into caller-owned, contiguous fp32 storage
 *     (int32/int64 where stated); shapes are int32.
 *   - activations are NHWC ("channels last") fp32 inside the library; the reference's
 *     NCHW tensors cross the boundary through seam_nchw_to_nhwc_f32 / seam_nhwc_to_nchw_f32.
 *   - thread-safe for distinct streams.
 *
 * Each entry cites the reference interface (file:line under the reference tree) whose
 * arithmetic it replaces.  "[TV]" = the arithmetic lives in torchvision, which the
 * reference only configures (models/video_matchrcnn.py:6-9,337-338).
 */
#ifndef SEAM_HIP_H
#define SEAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* seam_stream_t; /* hipStream_t */

/* ABI version (major*1000 + minor). */
int seam_version(void);
/* host helper: 1 when __umulhi(n, ceil(2^32 / d)) == n / d for every n < n_max (csrc/seam_fastdiv.h:
 * (n_max - 1) * (ceil(2^32 / d) * d - 2^32) < 2^32; d == 1 counts as exact, d == 0 never) -- the rule
 * every launcher applies before it hands a kernel such a multiplier */
int seam_fastdiv_exact(unsigned d, unsigned long long n_max);
/* hipGetErrorString for a code returned by any entry point. */
const char* seam_error_string(int code);

/* Variant selectors of the launchers (kernel-form switches the parity tests and the A/B tools flip: which Winograd form,
 * persistent or one tile per block, a forced implicit-GEMM tile ...).  A launcher never reads the environment; these are
 * process-wide ints, named like the environment variables the Python host applies once at load time ("SEAM_W24_PC", ...;
 * the table is csrc/seam_opts.h).  Every variant of a kernel computes the same results (bit-identical where the tests say so).
 * seam_set_option / seam_get_option return 0, or hipErrorInvalidValue for an unknown name. */
int seam_option_count(void);
const char* seam_option_name(int index);           /* NULL outside [0, count) */
int seam_set_option(const char* name, int value);
int seam_get_option(const char* name, int* value);

/* ---------------------------------------------------------------------------------
 * Implicit-GEMM convolution, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces every conv / linear on the path:
 *   ResNet-50 body + FrozenBN [TV]            (ctor models/video_matchrcnn.py:337)
 *   FPN lateral/output convs, RPNHead [TV]    (models/video_matchrcnn.py:337-338)
 *   TwoMLPHead / FastRCNNPredictor [TV]       (call models/video_matchrcnn.py:226-227)
 *   MaskRCNNHeads / MaskRCNNPredictor [TV]    (call models/video_matchrcnn.py:278-279)
 *   MatchPredictor.conv_seq / .linear         (models/match_head.py:50-62,67-69,93-95)
 *
 *   y[n,ho,wo,k] = act( scale[k] * sum_{r,s,c} x[n,ho*stride+r-pad,wo*stride+s-pad,c]
 *                                   * w[k][(r*S+s)*C+c]  + shift[k] + residual[n,ho,wo,k] )
 *
 * x        NHWC [N,H,W,C], C multiple of 4 and, when C >= 32, of 32 (pad channels zero-weighted)
 * w_packed rows_padded*kred floats from seam_pack_conv_weight_f32 (tile-contiguous slabs
 *          [n_tile][chunk][BN][32]; opaque to the caller)
 * scale    [K] or NULL (=1);  shift [K] or NULL (=0)   (bias / folded BatchNorm)
 * residual NHWC [N,Ho,Wo,K] or NULL, added before the activation
 * relu     0 none | 1 ReLU | 2 (backward passes) `residual` is NOT added: the result is zeroed where
 *          residual <= 0 -- the ReLU mask of the forward activation fused into the input-gradient conv
 * kred     padded reduction length = seam_conv_kred(C,R,S)
 * Refused (hipErrorInvalidValue, nothing launched), here and in every seam_conv2d_* form below: N <= 0, K <= 0, a C outside
 *          the rule above, stride < 1, and a kernel larger than the padded input (H + 2*pad < R or W + 2*pad < S:
 *          there is no output pixel, whatever the stride).  Any R, S, stride and pad inside that are served.
 */
int seam_conv_kred(int C, int R, int S);           /* host helper: ceil(R*S*C / 32) * 32 */
int seam_conv_rows_padded(int K);                  /* host helper: ceil(K / 64) * 64      */
int seam_conv_tile(int M, int K);                  /* host helper: BM*1000+BN of the block tile the fp32 launcher
                                                      picks for an [M x K] output (128 or 64 each) */
int seam_conv_tile_prec(int prec, int M, int K);   /* same for prec 0 = fp32, 1 = fp16, 2 = split-bf16 (these two also
                                                      have a 256x128 tile run by 8 waves) */
int seam_conv_tile_taps(int prec, int M, int K, int taps);   /* ... for a layer with R*S = taps (the fp16 choice depends on it) */

/* Pack an OIHW weight [K,Cin,R,S] (PyTorch layout) into the kernel's slab layout
 * (rows_padded*kred floats; reduction chunks ordered (r, c-chunk, s); channels >= Cin zero-filled).
 * mode 0: Conv2d / Linear (Linear = R=S=1; fc6 = a 7x7 "valid" conv over the 7x7 ROI tile)
 * mode 1: ConvTranspose2d(k=2,s=2) weight [Cin,Cout,2,2] -> rows ((a*2+b)*Cout + co),
 *         i.e. a 1x1 conv producing the 4 sub-pixels as channel groups; K = 4*Cout.
 * mode 2: input-gradient weights of a Conv2d whose OIHW weight is w [Cin, K, R, S] (note the roles:
 *         K = the forward conv's INPUT channels = rows produced, Cin = its output channels = channels
 *         reduced): taps rotated by 180 degrees, channels swapped, so that
 *         dX = seam_conv2d_f32(dY, packed, pad = R-1-pad_fwd) for a stride-1 conv (Linear: W^T).   */
int seam_pack_conv_weight_f32(const float* w, float* w_packed, int K, int Cin, int R, int S,
                              int Cstore, int mode, seam_stream_t stream);

int seam_conv2d_f32(const float* x, const float* w_packed, const float* scale,
                    const float* shift, const float* residual, float* y,
                    int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                    int relu, seam_stream_t stream);

/* The same convolution with the FPN top-down merge [TV FeaturePyramidNetwork.forward: inner_lateral +
 * F.interpolate(last_inner, size=feat_shape, mode="nearest")] fused into its epilogue (SURVEY 8b
 * `seam_fpn_topdown_add_f32`): y = act(conv(x)*scale + shift + top[n, floor(ho*Ht/Ho), floor(wo*Wt/Wo), :]),
 * top NHWC [N,Ht,Wt,K], K % 4 == 0.  Same rounding order as seam_conv2d_f32 followed by seam_upsample_add_f32
 * (bit-identical), without writing and re-reading the lateral map. */
int seam_conv2d_upres_f32(const float* x, const float* w_packed, const float* scale, const float* shift,
                          const float* top, float* y, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int Ht, int Wt, int relu, seam_stream_t stream);

/* seam_conv2d_f32 with the output grid cropped to its top-left [Ho, Wo] (Ho, Wo <= the full output size): `pad` rows /
 * columns of zeros before the map and fewer after it.  Call site: the ResNet stem [TV ResNet.conv1, 7x7 / stride 2 / pad 3]
 * on the space-to-depth input written by seam_preprocess_s2d_batch_f32 -- a 4x4 / stride-1 convolution over 12 channels
 * with 2 rows of padding before and 1 after (weights re-indexed on the host: w'[k,(dy,dx,c),r',s'] = w[k,c,2r'+dy-1,2s'+dx-1]). */
int seam_conv2d_crop_f32(const float* x, const float* w_packed, const float* scale, const float* shift, float* y,
                         int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int Ho, int Wo,
                         int relu, seam_stream_t stream);
/* fp16 twin (operands fp16, fp32 accumulate): the stem of the fp16 path on seam_preprocess_s2d_batch_f16's 16-channel cells. */
int seam_conv2d_crop_f16(const void* x, const void* w_packed, const float* scale, const float* shift, void* y,
                         int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int Ho, int Wo,
                         int relu, seam_stream_t stream);

/* ResNet downsample blocks [TV Bottleneck.forward: out = relu(bn3(conv3(h)) + bn_d(conv_d(x)))] as ONE GEMM over two 1x1
 * sources: y[n,ho,wo,:] = act(W[:, :C1] . x1[n,ho,wo,:] + W[:, C1:] . x2[n,ho*stride2,wo*stride2,:] (* scale) + shift).
 * x1 NHWC [N,Ho,Wo,C1], x2 NHWC [N,H2,W2,C2], C1 and C2 multiples of 32; w_packed = seam_pack_conv_weight_f32 of the
 * [K, C1+C2, 1, 1] weight (the host folds the two FrozenBN scales into it and adds the shifts).  The shortcut branch is
 * never written to memory and read back as a residual. */
int seam_conv2d_dual_f32(const float* x1, const float* x2, const float* w_packed, const float* scale,
                         const float* shift, float* y, int N, int Ho, int Wo, int C1, int H2, int W2, int C2,
                         int stride2, int K, int relu, seam_stream_t stream);

/* Pointwise (1x1, stride 1, pad 0) convolution with a SHORT reduction, weights stationary in LDS (csrc/seam_pw.hip) -- the same
 * contract as seam_conv2d_f32 / seam_conv2d_dual_f32 (stride2 = 1) / seam_conv2d_upres_f32 on those shapes [TV Bottleneck conv1 /
 * conv3, FeaturePyramidNetwork.inner_blocks, MaskRCNNPredictor.conv5_mask], exact fp32 on v_mfma_f32_32x32x2_f32:
 *   y[M,K] = act( [x | x2][M, C1 + C2] . w[K, C1 + C2]^T + shift [+ residual] )
 * x [M,C1], x2 [M,C2] or NULL (C2 = 0), w row-major [K, C1 + C2] with any per-channel scale already folded in (one fp32
 * rounding per weight), shift [K] (required).  res_mode 0: no residual; 1: residual [M,K]; 2: residual = coarse NHWC map
 * [N,rH,rW,K] added through a nearest-neighbour upsample to the [Ho,Wo] output grid (M = N*Ho*Wo, ATen's index rule).
 * Shapes served: C1, C2 multiples of 32, C1 + C2 <= 256, K a multiple of 64 (of 128 / 256 for the wider wave tiles), any M > 0;
 * seam_conv1x1_sw_config returns 0 for anything else (MT*100 + NT of the wave tile otherwise) and the launcher then returns
 * hipErrorInvalidValue.  An output pixel is one wave's fixed fma chain: results are deterministic and independent of M. */
int seam_conv1x1_sw_config(int M, int C1, int C2, int K);
int seam_conv1x1_sw_f32(const float* x, const float* x2, const float* w, const float* shift, const float* residual, float* y,
                        int M, int C1, int C2, int K, int relu, int res_mode, int Ho, int Wo, int rH, int rW,
                        seam_stream_t stream);

/* conv1x1_f16pc (csrc/seam_pwhpc.hip, round 6): the fp16 1x1 / stride-1 layers with a LONG reduction (C >= 512, a multiple of 256; K a
 * multiple of 128) as a producer / consumer block -- the fp16 twin of seam_conv1x1_pc_f32.  Replaces, for those shapes, the reference's
 * `torch.nn.Conv2d(C, K, 1)` + FrozenBatchNorm2d + ReLU of torchvision's Bottleneck.conv1 (reached from
 * /root/reference/models/video_matchrcnn.py:57-66 through `resnet_fpn_backbone`) under autocast-free fp16 operands.
 *   _supported: 1 when the shape is served;  _weight_halves: fp16 elements of the packed weights;
 *   seam_pack_conv1x1_weight_f16pc: w [K, C] fp32 row-major -> fragment order;
 *   seam_conv1x1_f16pc: y[M, K] = act(scale * (x[M, C] . w^T) + shift), fp16 in / out, fp32 accumulation; `residual` must be NULL. */
int seam_conv1x1_f16pc_supported(long long M, int C, int K);
long long seam_conv1x1_f16pc_weight_halves(int K, int C);
int seam_pack_conv1x1_weight_f16pc(const float* w, void* w_packed, int K, int C, seam_stream_t stream);
int seam_conv1x1_f16pc(const void* x, const void* w_packed, const float* scale, const float* shift, const void* residual, void* y,
                       long long M, int C, int K, int relu, seam_stream_t stream);

/* conv1x1_sxpc (csrc/seam_pwsx.hip): the fp32 1x1 / stride-1 / pad-0 layers with a long reduction as six-term split-bf16 products
 * (the arithmetic of seam_conv2d_sx with terms = 6, bit for bit) on a producer / consumer block -- the split twin of
 * seam_conv1x1_pc_f32.  Serves torchvision's Bottleneck.conv1 / conv3 + FrozenBatchNorm2d (+ residual) + ReLU on the fp32 path.
 *   _supported: 1 when the shape is served (C >= 256 and a multiple of 64, K a multiple of 128, M >= 1), else 0;
 *   _weight_bytes: bytes of the packed weights (three bf16 planes: 6 K C);
 *   seam_pack_conv1x1_weight_sxpc: w [K, C] fp32 row-major -> [K/128][4][C/16][3 planes][64 lanes][8 bf16] (no padding: the
 *   supported shapes have none);
 *   seam_conv1x1_sxpc: y[M, K] = act(scale * (x[M, C] . w^T) + shift + residual), fp32 in / out; relu 0 | 1; a shape that is not
 *   supported returns hipErrorInvalidValue and launches nothing. */
int seam_conv1x1_sxpc_supported(long long M, int C, int K);
long long seam_conv1x1_sxpc_weight_bytes(int K, int C);
int seam_pack_conv1x1_weight_sxpc(const float* w, void* w_packed, int K, int C, seam_stream_t stream);
int seam_conv1x1_sxpc(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                      long long M, int C, int K, int relu, seam_stream_t stream);

/* conv1x1_sxpc_dual (csrc/seam_pwsx.hip): the same kernel with a reduction over TWO sources -- torchvision's Bottleneck with a
 * projection shortcut, bn3(conv3(h)) + bn_d(conv_d(x)) + ReLU, as one GEMM over [x1 | x2 sampled at stride2] (the operands of
 * seam_conv2d_dual_f32).  x1 [N, Ho, Wo, C1], x2 [N, H2, W2, C2] read at (n, stride2 ho, stride2 wo); w_packed is
 * seam_pack_conv1x1_weight_sxpc of the [K, C1 + C2] matrix.  The result is bit for bit seam_conv1x1_sxpc on the materialised
 * concatenation; no residual.
 *   _supported: 1 when C1, C2 are multiples of 64 and (M, C1 + C2, K) is a shape of seam_conv1x1_sxpc_supported, else 0;
 *   seam_conv1x1_sxpc_dual: also needs stride2 >= 1, (Ho - 1) stride2 < H2, (Wo - 1) stride2 < W2, relu 0 | 1, and the images of
 *   x2 that one tile of 128 output pixels touches within 2 GiB (x2 itself may be any size); otherwise it returns
 *   hipErrorInvalidValue and launches nothing. */
int seam_conv1x1_sxpc_dual_supported(long long M, int C1, int C2, int K);
int seam_conv1x1_sxpc_dual(const float* x1, const float* x2, const void* w_packed, const float* scale, const float* shift, float* y,
                           int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int stride2, int K, int relu, seam_stream_t stream);

/* conv1x1_sxpc_up (csrc/seam_pwsx.hip): the same kernel with a nearest-upsampled coarse map as its residual -- torchvision's
 * FeaturePyramidNetwork lateral 1x1 (inner_blocks) plus the top-down merge, inner_lateral + F.interpolate(last_inner, size=...,
 * mode="nearest"), in one launch.  x [N, Ho, Wo, C], top [N, rH, rW, K] read at (n, nearest(ho), nearest(wo)) by ATen's rule
 * src = min(floor(dst * (float)in / (float)out), in - 1).  The result is bit for bit seam_conv1x1_sxpc (scale, shift, no residual,
 * no ReLU) followed by seam_upsample_add_f32 and, if asked, ReLU.
 *   _supported: 1 when (M, C, K) is a shape of seam_conv1x1_sxpc_supported, M == N Ho Wo, rH, rW >= 1, every grid side is below
 *   2^24 and the coarse images that one tile of 128 output pixels touches lie within 2 GiB (top itself may be any size), else 0;
 *   Wo == 1 and 1 x 1 maps are served;
 *   seam_conv1x1_sxpc_up: a null top, relu outside 0 | 1 or an unsupported geometry returns hipErrorInvalidValue and launches nothing. */
int seam_conv1x1_sxpc_up_supported(long long M, int N, int Ho, int Wo, int C, int K, int rH, int rW);
int seam_conv1x1_sxpc_up(const float* x, const void* w_packed, const float* scale, const float* shift, const float* top, float* y,
                         int N, int Ho, int Wo, int C, int K, int rH, int rW, int relu, seam_stream_t stream);

/* conv1x1_sxpc64 (csrc/seam_pwsx.hip): the same kernel for 64 output channels -- torchvision's Bottleneck.conv1 of layer1
 * (256 -> 64) and the base of the stem below.  A tile is 128 pixels x 64 channels; the four consumer waves own 32 channels x 64
 * pixels each.  Arithmetic and epilogue are seam_conv1x1_sxpc's: the bits of seam_conv2d_sx with terms = 6.
 *   _supported: 1 when K == 64, C >= 128 and a multiple of 64, M >= 1, else 0 (one chunk per tile, C == 64, is refused);
 *   seam_pack_conv1x1_weight_sxpc64: w [64, C] fp32 row-major -> [2][C/16][3 planes][64 lanes][8 bf16], 6 K C bytes
 *   (seam_conv1x1_sxpc_weight_bytes);
 *   seam_conv1x1_sxpc64: y[M, 64] = act(scale * (x[M, C] . w^T) + shift + residual); relu 0 | 1; a shape that is not supported
 *   returns hipErrorInvalidValue and launches nothing. */
int seam_conv1x1_sxpc64_supported(long long M, int C, int K);
int seam_pack_conv1x1_weight_sxpc64(const float* w, void* w_packed, int K, int C, seam_stream_t stream);
int seam_conv1x1_sxpc64(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                        long long M, int C, int K, int relu, seam_stream_t stream);

/* The `short` entries (csrc/seam_pwsx.hip): the kernels of seam_conv1x1_sxpc and seam_conv1x1_sxpc_dual on reductions of two
 * chunks, which the entries above refuse: C == 128 (torchvision's Bottleneck.conv3 of layer2, 128 -> 512 + residual) and
 * C1 == C2 == 64 on one map (layer1.0's conv3 + projection shortcut, stride2 == 1).  K a multiple of 128, M >= 1; the bits are those
 * of seam_conv2d_sx with terms = 6 (on the concatenated rows).  The pack is seam_pack_conv1x1_weight_sxpc's layout, 6 K C bytes.
 * Anything else returns hipErrorInvalidValue and launches nothing. */
int seam_conv1x1_sxpc_short_supported(long long M, int C, int K);
int seam_pack_conv1x1_weight_sxpc_short(const float* w, void* w_packed, int K, int C, seam_stream_t stream);
int seam_conv1x1_sxpc_short(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                            long long M, int C, int K, int relu, seam_stream_t stream);
int seam_conv1x1_sxpc_dual_short_supported(long long M, int C1, int C2, int K);
int seam_conv1x1_sxpc_dual_short(const float* x1, const float* x2, const void* w_packed, const float* scale, const float* shift, float* y,
                                 int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int K, int relu, seam_stream_t stream);

/* stem_sxpc (csrc/seam_pwsx.hip): torchvision's ResNet stem, conv1 (7x7 / stride 2 / pad 3) + FrozenBatchNorm2d + ReLU, in its
 * space-to-depth form -- the 4x4 / stride-1 convolution over the 12-channel frame -- as the gather form of conv1x1_sxpc64: an
 * output pixel's reduction is its 4 x 4 window of cells, 4 tap rows of 48 contiguous floats, three chunks of 64.  xp is the frame
 * with its zero cells, [N, Hs + 3, Ws + 3, 12] (2 before, 1 after in both directions); y [N, Hs, Ws, 64]; w_packed is
 * seam_pack_conv1x1_weight_sxpc64 of the [64, 192] rows in (r, s, c) order.  The result is bit for bit seam_conv1x1_sxpc64 on the
 * gathered [N Hs Ws, 192] rows.
 *   _supported: 1 when N, Hs, Ws >= 1, N Hs Ws < 2^31, the division rules hold and the frames that one tile of 128 output pixels
 *   touches lie within 2 GiB, else 0;
 *   seam_stem_sxpc: a null frame, relu outside 0 | 1 or an unsupported geometry returns hipErrorInvalidValue and launches nothing. */
int seam_stem_sxpc_supported(int N, int Hs, int Ws);
int seam_stem_sxpc(const float* xp, const void* w_packed, const float* scale, const float* shift, float* y, int N, int Hs, int Ws,
                   int relu, seam_stream_t stream);

/* fp16 twin of seam_conv1x1_sw_f32 (csrc/seam_pwh.hip, round 6): the config-5 path's 1x1 layers [TV Bottleneck conv1 / conv3 /
 * stride-1 projection shortcut, FeaturePyramidNetwork.inner_blocks; behind models/video_matchrcnn.py:337] as a STREAMING kernel --
 * weights stationary in LDS, independent waves, 16-byte NHWC pieces in and out -- with the contract of seam_conv2d_f16 /
 * seam_conv2d_dual_f16 (stride2 = 1) on those shapes:
 *   y[M,K] = fp16( act( [x | x2][M, C1 + C2] . w[K, C1 + C2]^T * scale + shift [+ residual] ) )
 * res_mode 0: no residual (residual NULL); 1: residual [M,K]; 2 (single source only): residual = coarse NHWC map [N,rH,rW,K] added
 * through a nearest-neighbour upsample to the [Ho,Wo] output grid (M = N*Ho*Wo, Ho*Wo >= 128; ATen's index rule) -- the FPN top-down
 * merge [TV FeaturePyramidNetwork.forward] in the conv epilogue, as seam_conv1x1_sw_f32 / seam_conv2d_upres_f32 do in fp32.
 * x, x2, residual, y fp16; w fp16 row-major [K, C1 + C2]; scale / shift fp32 [K] or NULL; fp32 accumulation, fp32 epilogue, one
 * rounding.  Shapes served (seam_conv1x1_swh_config != 0): C1, C2 multiples of 64, C1 + C2 <= 512 (<= 256 for the 256-channel slab
 * K % 256 == 0 takes, <= 128 when K is not a multiple of 128), K a multiple of 64 with K / slab dividing 32; any M > 0.  relu 0 | 1.  Same products as seam_conv2d_f16 in a
 * different accumulation order (agreement to fp32 rounding, not bit for bit); deterministic and independent of M. */
int seam_conv1x1_swh_config(long long M, int C1, int C2, int K);
int seam_conv1x1_swh_f16(const void* x, const void* x2, const void* w, const float* scale, const float* shift,
                         const void* residual, void* y, long long M, int C1, int C2, int K, int relu, int res_mode,
                         int Ho, int Wo, int rH, int rW, seam_stream_t stream);

/* The ResNet stem [TV ResNet.conv1 7x7 / stride 2 / pad 3 + bn1 + relu; behind models/video_matchrcnn.py:337] of the fp16 path on the
 * PADDED space-to-depth frame, as the streaming kernel above (csrc/seam_pwh.hip, round 6): xpad fp16 [N, Ho + 3, Wo + 3, 16] = the
 * frame of seam_preprocess_s2d_batch_f16 with 2 zero cells before and 1 after in both directions; w fp16 [64, 256] row-major with
 * k = (4 r + s) * 16 + channel (the re-indexed weights of seam_conv2d_crop_f16's call site); scale / shift fp32 [64] or NULL;
 * y fp16 [N, Ho, Wo, 64].  A tap is a constant shift of the flattened padded index, so every A fragment is one contiguous 1 KB run.
 * Same products as seam_conv2d_crop_f16, fp32 accumulation in tap-major order (agreement to fp32 rounding); deterministic. */
int seam_stem_s2d_swh_f16(const void* xpad, const void* w, const float* scale, const float* shift, void* y, int N, int Ho, int Wo,
                          int relu, seam_stream_t stream);

/* Pointwise (1x1, stride 1, pad 0) convolution with a LONG reduction as producer / consumer waves (csrc/seam_pwpc.hip, round 5):
 * the bottleneck reductions of ResNet layer2-4 and the layer4 expansions [TV Bottleneck conv1 / conv3 behind
 * models/video_matchrcnn.py:337], exact fp32 on v_mfma_f32_32x32x2_f32, the same contract as seam_conv2d_f32 on those shapes:
 *   y[M,K] = act( x[M,C] . W[K,C]^T * scale + shift [+ residual[M,K]] )
 * Shapes served (seam_conv1x1_pc_supported): C >= 256 and a multiple of 128, K a multiple of 128, any M > 0.  Weights:
 * seam_conv1x1_pc_weight_floats(K, C) floats from seam_pack_conv1x1_pc_f32 (row-major [K, C] in; MFMA fragment order).  scale /
 * shift [K] or NULL.  An output is one wave's fixed fma chain over k: results are deterministic and independent of M; they differ
 * from seam_conv2d_f32's by the order of the fp32 accumulation only. */
int seam_conv1x1_pc_supported(long long M, int C, int K);
long long seam_conv1x1_pc_weight_floats(int K, int C);
int seam_pack_conv1x1_pc_f32(const float* w, float* w_packed, int K, int C, seam_stream_t stream);
int seam_conv1x1_pc_f32(const float* x, const float* w_packed, const float* scale, const float* shift, const float* residual,
                        float* y, long long M, int C, int K, int relu, seam_stream_t stream);

/* fp16 twin of seam_conv2d_dual_f32 (x1, x2, w_packed, y fp16; C1 and C2 multiples of 64; fp32 accumulation and epilogue). */
int seam_conv2d_dual_f16(const void* x1, const void* x2, const void* w_packed, const float* scale,
                         const float* shift, void* y, int N, int Ho, int Wo, int C1, int H2, int W2, int C2,
                         int stride2, int K, int relu, seam_stream_t stream);

/* fp16 variant (BASELINE config 5: "fp16 MFMA path with fp32 ... accumulation"): x, w_packed,
 * residual are IEEE fp16 (NHWC, C multiple of 8 and, when C >= 64, of 64); v_mfma_f32_32x32x16_f16
 * with fp32 accumulators; scale/shift stay fp32; y is fp16, or fp32 when y_f32 != 0 (the last trunk
 * Linear hands fp32 descriptors to the fp32 heads).  Weights come from seam_pack_conv_weight_f16
 * (source still the fp32 OIHW parameter; rows_padded * seam_conv_kred_f16(C,R,S) halves). */
int seam_conv_kred_f16(int C, int R, int S);
int seam_pack_conv_weight_f16(const float* w, void* w_packed, int K, int Cin, int R, int S,
                              int Cstore, int mode, seam_stream_t stream);
int seam_conv2d_f16(const void* x, const void* w_packed, const float* scale, const float* shift,
                    const void* residual, void* y, int N, int H, int W, int C, int K, int R, int S,
                    int stride, int pad, int relu, int y_f32, seam_stream_t stream);

/* ---------------------------------------------------------------------------------
 * GeneralizedRCNNTransform [TV] (reached from GeneralizedRCNN.forward; callers
 * stuffs/engine.py:115, evaluate_movingfashion.py:31): per image
 *   (x-mean)/std -> bilinear resize (align_corners=False, scale=in/out) to [out_h,out_w]
 *   -> zero-pad to [Hp,Wp] -> NHWC with 4 stored channels (4th = 0).
 * img  CHW [3,in_h,in_w] in [0,1];  out NHWC4 slot [Hp,Wp,4] of the batch tensor. */
int seam_preprocess_f32(const float* img, float* out, int in_h, int in_w, int out_h, int out_w,
                        int Hp, int Wp, seam_stream_t stream);

int seam_preprocess_f16(const float* img, void* out /* fp16 NHWC8 */, int in_h, int in_w, int out_h,
                        int out_w, int Hp, int Wp, seam_stream_t stream);

/* The same transform for n images of ONE shape laid out at a constant stride (img_stride floats between
 * consecutive images: the frames of a clip tensor [T,3,H,W], which the reference hands over as a list of views):
 * one launch writes the whole NHWC batch [n,Hp,Wp,4] (fp16: [n,Hp,Wp,8]).  n <= 65535. */
int seam_preprocess_batch_f32(const float* imgs, size_t img_stride, float* out, int n, int in_h, int in_w,
                              int out_h, int out_w, int Hp, int Wp, seam_stream_t stream);
int seam_preprocess_batch_f16(const float* imgs, size_t img_stride, void* out, int n, int in_h, int in_w,
                              int out_h, int out_w, int Hp, int Wp, seam_stream_t stream);

/* The same transform written space-to-depth for the stem: out [n, Hp/2, Wp/2, 12], channel (dy*2+dx)*3 + c = pixel
 * (2Y+dy, 2X+dx), colour c (Hp, Wp even). */
int seam_preprocess_s2d_batch_f32(const float* imgs, size_t img_stride, float* out, int n, int in_h, int in_w,
                                  int out_h, int out_w, int Hp, int Wp, seam_stream_t stream);
/* fp16 output: [n, Hp/2, Wp/2, 16] -- the 12 channels above + 4 zeros (the fp16 GEMM reads 8-channel vectors). */
int seam_preprocess_s2d_batch_f16(const float* imgs, size_t img_stride, void* out, int n, int in_h, int in_w,
                                  int out_h, int out_w, int Hp, int Wp, seam_stream_t stream);
/* The same frame with pad_lo zero cells before and pad_hi after it in both directions: out [n, Hp/2 + pad_lo + pad_hi,
 * Wp/2 + pad_lo + pad_hi, 16] -- the input layout of seam_stem_s2d_swh_f16 (pad_lo 2, pad_hi 1: the 4x4 / pad-2 form of the stem). */
int seam_preprocess_s2d_pad_batch_f16(const float* imgs, size_t img_stride, void* out, int n, int in_h, int in_w, int out_h,
                                      int out_w, int Hp, int Wp, int pad_lo, int pad_hi, seam_stream_t stream);
/* fp32 twin: out [n, Hp/2 + pad_lo + pad_hi, Wp/2 + pad_lo + pad_hi, 12] -- the input layout of seam_stem_sxpc (pad_lo 2, pad_hi 1);
 * the interior is seam_preprocess_s2d_batch_f32's frame bit for bit. */
int seam_preprocess_s2d_pad_batch_f32(const float* imgs, size_t img_stride, float* out, int n, int in_h, int in_w, int out_h,
                                      int out_w, int Hp, int Wp, int pad_lo, int pad_hi, seam_stream_t stream);

/* Same transform fed by a uint8 HWC RGB frame [in_h,in_w,3]: fuses ToTensor (x/255, stuffs/transform.py:46-49)
 * so a clip crosses PCIe at 1 byte per sample (device side).  out: fp32 NHWC4 or, when
 * out_f16 != 0, fp16 NHWC8. */
int seam_preprocess_u8(const uint8_t* img, void* out, int in_h, int in_w, int out_h, int out_w,
                       int Hp, int Wp, int out_f16, seam_stream_t stream);

/* max_pool2d on NHWC [TV: ResNet stem 3x3/s2/p1; LastLevelMaxPool k=1,s=2]. C % 4 == 0. */
int seam_maxpool2d_f32(const float* x, float* y, int N, int H, int W, int C, int k, int stride,
                       int pad, seam_stream_t stream);

int seam_maxpool2d_f16(const void* x, void* y, int N, int H, int W, int C, int k, int stride,
                       int pad, seam_stream_t stream);   /* fp16, C % 8 == 0 */
/* host helper: 1 when the launcher takes the 3x3/s2/p1 kernel with 32-bit multiply-high index
 * divisions (both exact by seam_fastdiv_exact), 0 when it takes the generic 64-bit kernel */
int seam_maxpool2d_fast(int N, int H, int W, int C, int k, int stride, int pad, int f16);

/* FPN top-down [TV]: lat[n,h,w,:] += top[n, floor(h*Ht/H), floor(w*Wt/W), :] (nearest). */
int seam_upsample_add_f32(float* lat, const float* top, int N, int H, int W, int Ht, int Wt, int C,
                          seam_stream_t stream);

int seam_upsample_add_f16(void* lat, const void* top, int N, int H, int W, int Ht, int Wt, int C,
                          seam_stream_t stream);

/* ---------------------------------------------------------------------------------
 * MultiScaleRoIAlign(['0','1','2','3'], P, sampling_ratio) + roi_align(aligned=False) [TV]
 * call sites models/video_matchrcnn.py:225 (P=7), :277 (P=14); models/matchrcnn.py:463.
 * feat[l] NHWC [N,Hl,Wl,C] (C % 4 == 0, C <= 1024);  rois [K,5] = (batch_idx,x1,y1,x2,y2)
 * in resized-image pixels;  levels int32 [K] or NULL (NULL: LevelMapper on device:
 * clamp(floor(4+log2(sqrt(area)/224)+1e-6), k_min, k_min+3) - k_min);
 * scales[l] = 2^round(log2(Hl/Himg)) passed by value;  out NHWC [K,P,P,C]. */
int seam_roi_align_f32(const float* feat0, const float* feat1, const float* feat2, const float* feat3,
                       const int* hw /* host int[8]: H0,W0,...,H3,W3 */, int C,
                       float scale0, float scale1, float scale2, float scale3, int k_min,
                       const float* rois, const int* levels, float* out, int K, int P,
                       int sampling_ratio, seam_stream_t stream);

int seam_roi_align_f16(const void* feat0, const void* feat1, const void* feat2, const void* feat3,
                       const int* hw, int C, float scale0, float scale1, float scale2, float scale3,
                       int k_min, const float* rois, const int* levels, void* out, int K, int P,
                       int sampling_ratio, seam_stream_t stream);   /* fp16 maps in, fp16 out */

/* TEST / BENCHMARK HOOK ONLY -- not part of the per-stream thread-safety contract of this header: a process-wide selector of the
 * kernel the two entry points above launch (also env SEAM_ROIALIGN_LDS at first use): 2 (default) = LDS-staged ROI quadrant tiles,
 * 1 = row-staged tiles, 0 = one wave per bin gathering its 16 taps from L1/L2 (also what any shape outside sampling_ratio 2,
 * P <= 16, C % 64 == 0 takes).  All three give bit-identical results, so a concurrent change can never alter an output -- but
 * production callers should not call it (tools/roialign_ab.py and tests/test_gpu_ops.py do); measurements in
 * profiles/r03_roialign_ab.txt. */
void seam_roi_align_set_lds(int on);

/* Layout bridges at the module boundary: x [B,C,L] <-> y [B,L,C]. */
int seam_nchw_to_nhwc_f32(const float* x, float* y, int B, int C, int L, seam_stream_t stream);
int seam_nhwc_to_nchw_f32(const float* x, float* y, int B, int L, int C, seam_stream_t stream);

/* fp16 path: the reference-facing side stays fp32 NCHW, the library side is fp16 NHWC. */
int seam_nchw_f32_to_nhwc_f16(const float* x, void* y, int B, int C, int L, seam_stream_t stream);
int seam_nhwc_f16_to_nchw_f32(const void* x, float* y, int B, int L, int C, seam_stream_t stream);

/* AvgPool2d((6,6)) (+ no-op ReLU) of models/match_head.py:59-60: x [K,L,C] -> y [K,C]. */
int seam_avgpool_f32(const float* x, float* y, int K, int L, int C, seam_stream_t stream);

int seam_avgpool_f16(const void* x, void* y, int K, int L, int C, seam_stream_t stream);

/* ---------------------------------------------------------------------------------
 * NONLocalBlock1D(256, sub_sample=False, bn_layer=False) + attention pooling, batched
 * over sequences: models/nlb.py:66-101 via models/match_head.py:114-121 / :144-151.
 *   per sequence X[T,256]:  TH/PH/G = X W^T + b ; a = TH.wc[:128] ; b = PH.wc[128:]
 *   f = ReLU(a_i+b_j)/T ; Y = f G ; Z = Y Ww^T + bw + X      (T == 1: Z = X, ref :115-117)
 *   s = Z.wa + ba ; p = softmax_t(s) ; out = sum_t p_t Z_t   (T == 0: out = 0)
 * seq      element (t,s,c) at seq[t*t_stride + s*s_stride + c], t < len[s]
 *          (pass x3_1_seq + S*256, t_stride = S*256, s_stride = 256: row 0 is the dummy)
 * len      int32 [S] (device)
 * w_proj_t [256][384] = concat(theta,phi,g).weight transposed;  b_proj [384]
 * w_cat    [256] concat_project weight;  w_out_t [128][256] = W.weight^T;  b_out [256]
 * w_att [256], b_att [1]
 * out [S,256];  att [S,Tmax] or NULL (softmax weights; entries >= len[s] untouched)
 * z   [S,Tmax,256] or NULL: the non-local block's own output Z (= NONLocalBlock1D.forward)
 * ws   workspace, >= seam_nlb_workspace_floats(S,Tmax) floats
 * use_nlb  0: no block; 1: the module's `.nlb` flag (models/match_head.py:88), length-1
 *          sequences bypass the block (ref :115-117); 2: apply the block to every sequence */
int64_t seam_nlb_workspace_floats(int S, int Tmax);
int seam_nlb_attnpool_f32(const float* seq, int64_t t_stride, int64_t s_stride, const int* len,
                          int S, int Tmax, const float* w_proj_t, const float* b_proj,
                          const float* w_cat, const float* w_out_t, const float* b_out,
                          const float* w_att, const float* b_att, float* out, float* att,
                          float* z, float* ws, int use_nlb, seam_stream_t stream);

/* The same block with its GEMMs on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32): G = X Wg + bg, Y = f G and
 * Z = Y Ww^T + bw + X per 32-row tile, one workgroup per sequence, sequences of at most seam_nlb_mfma_max_len() (96) rows;
 * seq rows 16-byte aligned (t_stride, s_stride multiples of 4 floats).  theta / phi enter the block only through
 * a_i = theta_i . wc[:128] and b_j = phi_j . wc[128:] (models/nlb.py:80-90), so the caller folds them once:
 *   u[256] = W_theta^T wc[:128], v[256] = W_phi^T wc[128:], cd[2] = (b_theta . wc[:128], b_phi . wc[128:]).
 * wg_frag [4][32][64][4] / wo_frag [8][16][64][4]: the g and W projections in MFMA B-fragment order -- element e of lane
 * (h = lane >> 5, n = lane & 31) of fragment [n_tile][j] = W[k = 8 j + 4 h + e][32 n_tile + n] (W as [k][n]).
 * out / att / z / use_nlb as above. */
int seam_nlb_mfma_max_len(void);
int seam_nlb_attnpool_mfma_f32(const float* seq, int64_t t_stride, int64_t s_stride, const int* len, int S, int Tmax,
                               const float* wg_frag, const float* b_g, const float* u, const float* v,
                               const float* cd, const float* wo_frag, const float* b_out, const float* w_att,
                               const float* b_att, float* out, float* att, float* z, int use_nlb,
                               seam_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Pairwise match classifier `last((a_i - b_j)^2)`: models/match_head.py:73-74,161-162;
 * NumPy twin evaluate_movingfashion.py:94-100,263-264.
 * a [Q,D], b [G,D], w [2,D], bias [2] -> out [Q,G,2].   D % 32 == 0, D <= 1024. */
int seam_pair_logits_f32(const float* a, const float* b, const float* w, const float* bias,
                         float* out, int Q, int G, int D, seam_stream_t stream);

/* Score + rank: evaluate_movingfashion.py:97-99,265-269.  Reads logits [Q,G,2]; ranks by
 * softmax(x)[...,1] (== monotone in x1-x0), descending, ties -> lower index first.
 * idx int64 [Q,k], score [Q,k] = softmax(x)[...,1] of the selected entries.
 * k <= G, k <= seam_rank_topk_max_k() (256): the selection keeps its winners in on-chip memory; a larger k is refused with
 * hipErrorInvalidValue and nothing is launched or written (a full ranking is what seam_rank_of_f32 is for).
 * NaN differences rank last (as -inf), -0 ties with +0. */
int seam_rank_topk_max_k(void);
int seam_rank_topk_f32(const float* logits, int64_t* idx, float* score, int Q, int G, int k,
                       seam_stream_t stream);

/* Evaluator-side scoring.  score = softmax(logits)[...,1] for n_pairs rows of 2
 * (compute_distances / compute_selfdist, evaluate_movingfashion.py:102-121);  rank[q] = position of
 * product target[q] in the descending ranking of query q (what `(rankings == shop_prod_index)
 * .nonzero()` extracts at evaluate_movingfashion.py:228,268), same tie rule as seam_rank_topk_f32. */
int seam_match_scores_f32(const float* logits, float* score, int64_t n_pairs, seam_stream_t stream);
/* HOST helper (host pointers, no device work, no stream): the greedy tracklet linking of evaluate_movingfashion.py:166-202 for all
 * products of an evaluator pass.  blocks = the products' n_s x n_s self-similarity blocks concatenated (what
 * seam_pair_scores_blockdiag_f32 wrote, copied to the host); seg int64 [n_seg + 1] detection offsets; imgs int64 / scores double
 * [seg[n_seg]] frame index / confidence per detection.  Out: members_out [seg[n_seg]] -- per product, at seg[s], the LOCAL detection
 * indices tracklet after tracklet (creation order), members in link order; track_len_out [seg[n_seg]] -- at seg[s] the lengths of
 * that product's tracklets; n_tracks_out [n_seg].  Same decisions as the reference's loops (first maximum in row-major order). */
int seam_host_build_tracklets(const float* blocks, const int64_t* seg, const int64_t* imgs, const double* scores, int n_seg,
                              double threshold, int32_t* members_out, int32_t* track_len_out, int32_t* n_tracks_out);

/* DEVICE twin of seam_host_build_tracklets (device pointers, one launch for all segments, one block per segment; no host
 * synchronisation): blocks / block_off (int64 [n_seg + 1]) / seg (int32 [n_seg + 1]) exactly as seam_pair_scores_blockdiag_f32 takes
 * and writes them; imgs int32 [rows] the frame label of every detection (compared for equality only: need be neither dense nor
 * sorted), scores fp32 [rows] the confidences; max_rows >= every n_s.  Out, int32, in the host helper's layout: members [rows],
 * track_len [rows] (entries from n_tracks[s] on are written as 0), n_tracks [n_seg], and track_of [rows], the tracklet number of every
 * detection; every element of those ranges is written.  Same decisions as the host helper on finite inputs (seed = most confident
 * free detection, lowest index among equals; candidate = first maximum of members x candidates in row-major order, members in
 * ascending detection order; sim[member][candidate] is read, the matrix need not be symmetric), except that the link test is
 * (double)value > threshold in fp64, where the host helper compares with (float)threshold: float(0.3) links at 0.3 here.
 * Comparisons only, no float atomics: exact and deterministic.  NaN inputs: unspecified decisions, but the kernel terminates and
 * writes a partition.  seam_build_tracklets_max_rows(): the largest n_s served (the state lives in LDS).  Refused with
 * hipErrorInvalidValue, nothing launched or written: n_seg < 0, max_rows < 0 or above the cap, a NULL block_off / seg / n_tracks, and
 * any other NULL pointer when max_rows > 0.  n_seg == 0: no-op.  An empty segment: n_tracks[s] = 0.  A segment longer than
 * max_rows: untouched except n_tracks[s] = -1. */
int seam_build_tracklets_max_rows(void);
int seam_build_tracklets_f32(const float* blocks, const int64_t* block_off, const int* seg, const int* imgs, const float* scores,
                             int n_seg, int max_rows, double threshold, int32_t* members, int32_t* track_len, int32_t* n_tracks,
                             int32_t* track_of, seam_stream_t stream);

/* Block-diagonal self-similarity for the evaluator's tracking step (`compute_selfdist` once per product,
 * evaluate_movingfashion.py:102-121,165-176) in ONE launch: x [rows, Dd] holds the detections' descriptors grouped by product,
 * seg int32 [n_seg + 1] the group boundaries (row offsets), out_off int64 [n_seg + 1] the running sum of n_s^2; for every group
 * out[out_off[s] + i * n_s + j] = softmax(W (x_i - x_j)^2 + b)[1].  Only the n_s x n_s diagonal blocks are computed (the all-pairs
 * matrix of a pass is rows^2).  max_rows >= every n_s.  Bit-identical to seam_pair_logits_f32 + seam_match_scores_f32 per group. */
int seam_pair_scores_blockdiag_f32(const float* x, const int* seg, const int64_t* out_off, const float* w, const float* bias,
                                   float* out, int n_seg, int max_rows, int Dd, seam_stream_t stream);
int seam_rank_of_f32(const float* logits, const int64_t* target, int64_t* rank, int Q, int G,
                     seam_stream_t stream);

/* Rankings over per-frame score rows (evaluate_movingfashion.py:293-315): out[g] = mean (mode 0) or max
 * (mode 1) over the n rows of score [n,G];  seam_rank_of_scores_f32: rank of target[q] in the descending
 * order of the plain score row q of [Q,G] (ties -> lower index first; what `np.argsort(x)[::-1] ==
 * shop_prod_index` extracts at :296-297,306-307).
 * Edge behaviour (pinned by the tests): a NaN score makes the column's mean NaN and is ignored by the max (a column of
 * nothing but NaN gives -inf); n <= 0 and a mode other than 0 / 1 are refused with hipErrorInvalidValue. */
int seam_score_reduce_f32(const float* score, float* out, int n, int G, int mode, seam_stream_t stream);
/* ... over row segments: rows seg[p] .. seg[p+1]-1 (seg: P+1 int32 offsets on the device) -> out [P,G], one launch for all
 * products of an evaluator pass; bit-identical to P calls of seam_score_reduce_f32 (P <= 65535, more is refused).
 * An empty segment (seg[p] == seg[p+1]) is not refused: its row of out is NaN (mean, 0 / 0) or -inf (max). */
int seam_score_reduce_seg_f32(const float* score, const int* seg, float* out, int P, int G, int mode, seam_stream_t stream);
int seam_rank_of_scores_f32(const float* score, const int64_t* target, int64_t* rank, int Q, int G,
                            seam_stream_t stream);

/* torchvision.ops.box_iou as the evaluator calls it to pick the tracklet that follows the ground truth
 * (evaluate_movingfashion.py:205-209): a [Na,4], b [Nb,4] xyxy -> out [Na,Nb]. */
int seam_box_iou_f32(const float* a, const float* b, float* out, int Na, int Nb, seam_stream_t stream);

/* Multi-DeepFashion2 ground-truth selection (evaluate_multiDF2.py:43-57,75-89), one launch for the N images of a product:
 * in image n (detections det_off[n] .. det_off[n+1]-1 of det_boxes [Dtot,4] xyxy / det_scores [Dtot], GT boxes
 * gt_off[n] .. gt_off[n+1]-1 of gt_boxes [Gtot,4] xyxy) the detection with score >= score_threshold whose pycocotools
 * bbIou with GT row gt_row[n] (negative = from the end) is largest, first maximum over the thresholded subsequence.
 * sel_idx[n]: index into the image's full detection list, sel_pos[n]: position inside the kept subsequence; both -1 when
 * nothing is kept or status[n] != 0.  status[n]: 0, 1 = the image has no GT box, 2 = gt_row outside its GT rows (the GT is
 * only consulted when some detection is kept).  det_off / gt_off: N+1 int32 offsets on the device. */
int seam_gt_select_f32(const float* det_boxes, const float* det_scores, const int* det_off, const float* gt_boxes,
                       const int* gt_off, const int* gt_row, float score_threshold, int* sel_idx, int* sel_pos, int* status,
                       int N, seam_stream_t stream);

/* Fused pairwise logits + top-k (a13 + a14 in one pass; no [Q,G,2] round trip through HBM):
 * same ranking rule and bit-identical x1-x0 as seam_pair_logits_f32 + seam_rank_topk_f32.
 * k <= seam_rank_topk_max_k() (256), k <= G; ws: >= seam_pair_topk_workspace_floats(Q,G,k) floats of scratch. */
int64_t seam_pair_topk_workspace_floats(int Q, int G, int k);
int seam_pair_topk_f32(const float* a, const float* b, const float* w, const float* bias,
                       int64_t* idx, float* score, int Q, int G, int D, int k, float* ws,
                       seam_stream_t stream);

/* The same ranking for a LARGE bank (configs[2]/[3]: G = 20 000 / 50 000) on the fp32 matrix cores: candidates are found with the
 * expanded form of the logit difference (one [Q,256] x [256,G] v_mfma_f32_16x16x4_f32 GEMM + two rank-1 terms, per-query
 * threshold from a 4096-row sample, no [Q,G] tensor in HBM), the k + margin best are re-scored with the direct form in the
 * operation order of seam_pair_logits_f32, and a per-query rounding-error bound proves that no other product can enter the top k
 * (a query that fails the proof is redone with the direct form over the whole bank).  idx / score are bit-identical to
 * seam_pair_logits_f32 + seam_rank_topk_f32 (ref models/match_head.py:161-162; evaluate_movingfashion.py:94-100,263-269).
 * Requires D == 256, G >= seam_pair_topk_mfma_min_gallery(), k <= seam_pair_topk_mfma_max_k(), 16-byte aligned a / b / ws;
 * ws: >= seam_pair_topk_mfma_workspace_floats(Q,G,k) floats.  flags bit 0: direct-form path for every query (test hook).
 * stats: device int[4] or NULL -- [0] queries that took the direct-form path, [1] largest candidate count, [2] overflowed lists. */
int seam_pair_topk_mfma_min_gallery(void);
int seam_pair_topk_mfma_max_k(void);
int64_t seam_pair_topk_mfma_workspace_floats(int Q, int G, int k);
int seam_pair_topk_mfma_f32(const float* a, const float* b, const float* w, const float* bias,
                            int64_t* idx, float* score, int Q, int G, int D, int k, float* ws, int flags,
                            int* stats, seam_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Detection post-processing [TV] + models/video_matchrcnn.py:154-205.
 * BoxCoder.decode (weights wx,wy,ww,wh; dw,dh clamped to log(1000/16)) + clip to image.
 * deltas [N,ncls*4], anchors/proposals [N,4] -> boxes [N,ncls*4]. */
int seam_decode_boxes_f32(const float* deltas, const float* boxes_in, float* boxes_out, int N,
                          int ncls, float wx, float wy, float ww, float wh, float clip_h,
                          float clip_w, seam_stream_t stream);

/* Greedy NMS, batched over B images, over boxes [B,N,4] ALREADY SORTED by descending score inside
 * each image: keep[b,i]=1/0 (int32 [B,N]).  IoU > thr suppresses (strict), areas without +1.
 * 64x64 bitmask tiles + one-wave scan per image, N <= 16384.
 * mask_ws: uint64 workspace of B*N*ceil(N/64) words. */
int seam_nms_sorted_f32(const float* boxes, int* keep, int B, int N, float thr, uint64_t* mask_ws,
                        seam_stream_t stream);

/* Same, stopping after the first max_keep survivors of each image (0 = no limit): greedy NMS decides a box from
 * higher-scored boxes only, so the result equals the full scan truncated to max_keep survivors -- what the callers keep
 * anyway ([TV] filter_proposals post_nms_top_n; postprocess_detections detections_per_img,
 * models/video_matchrcnn.py:199-201). */
int seam_nms_sorted_topn_f32(const float* boxes, int* keep, int B, int N, float thr, int max_keep,
                             uint64_t* mask_ws, seam_stream_t stream);

/* RPN filter_proposals, per pyramid level [TV RegionProposalNetwork._get_top_n_idx + BoxCoder.decode + clip + sigmoid]
 * (SURVEY.md 8b `seam_rpn_decode_topk`): for each of n_img images the exact top-k of its n = H*W*A objectness logits
 * (logit descending, anchor index ascending = the first k of a stable descending sort), and for the winners in that order
 * the decoded (weights 1,1,1,1), clipped box, sigmoid(logit) and (optionally, index != NULL) the anchor index.
 * obj / deltas are read in place from the head output: logit of anchor j = (pixel j / A, a = j % A) at
 * obj[img*obj_img_stride + pixel*obj_pix_stride + a], its deltas at deltas[img*dlt_img_stride + pixel*dlt_pix_stride + 4a ..].
 * anchors [n,4]; clip_hw [n_img,2] = (height, width) of each resized image; outputs are written at row
 * img*out_img_stride + out_offset + rank (boxes [.,4], scores [.], index [.] int64).  k <= seam_rpn_topk_max() (1024), k <= n. */
int seam_rpn_topk_max(void);
int seam_rpn_topk_decode_f32(const float* obj, const float* deltas, const float* anchors,
                             const float* clip_hw, float* boxes, float* scores, int64_t* index,
                             int n_img, int n, int A, int k, int64_t obj_img_stride,
                             int obj_pix_stride, int64_t dlt_img_stride, int dlt_pix_stride,
                             int64_t out_img_stride, int out_offset, seam_stream_t stream);

/* paste_masks_in_image [TV] (transform.postprocess, reached from model(images)): masks [K,1,28,28]
 * probabilities, boxes [K,4] (original-image px) -> out [K,1,H,W]. */
int seam_paste_masks_f32(const float* masks, const float* boxes, float* out, int K, int H, int W,
                         seam_stream_t stream);

/* Mask intersections for COCO-style segm AP (evaluator_det.py), without the paste.  The mask of detection d is the set of
 * image pixels where seam_paste_masks_f32(probs, boxes) would write a value > 0.5 (strict; bit for bit: both kernels take
 * the value from one device function).  probs [D,28,28] (the selected-class probabilities of seam_mask_select_*),
 * boxes [D,4] xyxy in pixels of the original image, gt [G,H,W] uint8 (a pixel is set iff its byte != 0) ->
 * inter [D,G] = pixels set in both, det_area [D] = pixels set in the detection's mask inside the image.  Only the pixels
 * of each clipped integer box are visited: sum_d box_area_d x G byte reads, nothing image-sized is written.  Both outputs
 * are zeroed on the stream and accumulated with integer atomics, so repeated launches give identical results.
 * D == 0: no-op, returns 0.  G == 0: only det_area is written; inter and gt may be NULL.  A NULL required pointer, a
 * negative size or H*W >= 2^31 returns non-zero and writes nothing.  Degenerate, inverted and off-image boxes give what
 * the paste gives (usually no pixel) and read nothing outside gt. */
int seam_mask_inter_f32(const float* probs, const float* boxes, int D, const uint8_t* gt, int G, int H,
                        int W, int* inter, int* det_area, seam_stream_t stream);

/* maskrcnn_inference [TV] (call models/video_matchrcnn.py:291): logits laid out
 * [K,14,14,(a,b),ncls] (sub-pixel groups from the transposed conv) -> prob [K,1,28,28] of the
 * channel labels[k] (int64), after sigmoid. */
int seam_mask_select_f32(const float* logits, const int64_t* labels, float* prob, int K, int ncls,
                         seam_stream_t stream);

int seam_mask_select_f16(const void* logits, const int64_t* labels, float* prob, int K, int ncls,
                         seam_stream_t stream);   /* fp16 logits in, fp32 probabilities out */

/* ---------------------------------------------------------------------------------------------------
 * Split-bf16 ("bx3") convolution: the same contraction as seam_conv2d_f32 on fp32 activations, computed as
 * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with v_mfma_f32_32x32x16_bf16 and fp32 accumulation (relative error ~1e-5 per
 * product, fp32 exponent range; well inside the 1e-3 contract of BASELINE.json).  Same call sites as
 * seam_conv2d_f32 (opt-in: model.set_compute_dtype("bf16x3")).  Weights: seam_pack_conv_weight_bx3 (same size as
 * the fp32 pack; tmp = rows_padded*kred floats of scratch). */
int seam_pack_conv_weight_bx3(const float* w, void* w_packed, float* tmp, int K, int Cin, int R, int S,
                              int Cstore, int mode, seam_stream_t stream);
int seam_conv2d_bx3(const float* x, const void* w_packed, const float* scale, const float* shift,
                    const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                    int stride, int pad, int relu, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Three-plane split ("sx") convolution: the fp32 product on the bf16 matrix pipe.  Each fp32 operand is cut by
 * truncation into three bf16 pieces that sum back to it exactly (a = a0 + a1 + a2); every piece product is exact in
 * the fp32 accumulator.  terms = 6 keeps the products with i + j <= 2 (what is dropped is < 2^-22 of the product, one
 * fp32 rounding); terms = 9 keeps all nine (the exact fp32 product, summed in another order than the fma chain).
 * Same contraction, epilogue (scale / shift, residual, ReLU) and argument meaning as seam_conv2d_f32.  Inf / NaN
 * inputs give NaN outputs; inputs below 2^-110 lose bits under 2^-133.  Weights: seam_pack_conv_weight_sx
 * (rows_padded * kred * 6 bytes, three bf16 planes per chunk; tmp = rows_padded*kred floats of scratch). */
int seam_pack_conv_weight_sx(const float* w, void* w_packed, float* tmp, int K, int Cin, int R, int S,
                             int Cstore, int mode, seam_stream_t stream);
int seam_conv2d_sx(const float* x, const void* w_packed, const float* scale, const float* shift,
                   const float* residual, float* y, int N, int H, int W, int C, int K, int R, int S,
                   int stride, int pad, int relu, int terms, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Winograd F(2x2,3x3) convolution, fp32 MFMA: the stride-1 3x3 layers of the same call sites as seam_conv2d_f32
 * (ResNet-50 bottleneck 3x3s, FPN output convs, RPNHead conv [TV]; MaskRCNNHeads [TV]; MatchPredictor.conv_seq,
 * models/match_head.py:50-60) with 2.25x fewer matrix-core issues.  Same contract as seam_conv2d_f32 with R = S = 3,
 * stride = 1 (x NHWC [N,H,W,C], y NHWC [N,H+2*pad-2,W+2*pad-2,K], scale / shift / residual / relu identical);
 * C must be a multiple of 8 and K of 32 (seam_wino_supported).  All arithmetic is fp32; results differ from
 * seam_conv2d_f32 only by the rounding of the +/- transforms (~1e-6 relative to the output scale).
 * u_packed: seam_wino_weight_floats(K, Cstore) floats from seam_pack_conv_weight_wino_f32 (U = G g Gt per (k, c),
 * computed in fp64 and rounded once, stored in MFMA fragment order; mode 0 = forward weights [K,Cin,3,3],
 * mode 2 = input-gradient weights as in seam_pack_conv_weight_f32). */
int seam_wino_supported(int C, int K, int R, int S, int stride);
long long seam_wino_weight_floats(int K, int Cstore);
int seam_wino_slot_fill_pct(int N, int H, int W, int C, int K, int pad);   /* host helper: % of the launch's 2x2-tile slots
                                                                             that hold real output (the caller's switch
                                                                             between this kernel and seam_conv2d_f32) */
int seam_wino_tile_variant(int N, int H, int W, int C, int K, int pad);   /* host helper: MT of the conv3x3_wino<MT>
                                                                            kernel the launcher picks (32*MT tiles per block) */
int seam_pack_conv_weight_wino_f32(const float* w, float* u_packed, int K, int Cin, int Cstore, int mode,
                                   seam_stream_t stream);
int seam_conv3x3_wino_f32(const float* x, const float* u_packed, const float* scale, const float* shift,
                          const float* residual, float* y, int N, int H, int W, int C, int K, int pad, int relu,
                          seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 1x1 convolutions / Linear layers with at most 16 outputs (csrc/seam_narrow.hip): y[M,K] = act(x[M,C] . w[K,C]^T + bias),
 * C a multiple of 16, C <= 256, K <= 16 (seam_linear_narrow_supported).  Call sites: RPNHead.cls_logits + bbox_pred [TV]
 * (3 + 12 outputs per pixel, packed as one [15, 256] weight) and MaskRCNNPredictor.mask_fcn_logits [TV] (14 classes).
 * HBM-bound row stream on v_mfma_f32_16x16x4_f32 with the weights register-resident; w_packed = a buffer of 64 * C floats
 * from seam_pack_linear_narrow_f32 (source: the fp32 [K, C] weight), which writes -- and the kernel reads -- its first 16 * C
 * floats ([C / 16][64 lanes][4]) and leaves the rest alone. */
int seam_linear_narrow_supported(int C, int K);
int seam_pack_linear_narrow_f32(const float* w, float* w_packed, int K, int C, seam_stream_t stream);
int seam_linear_narrow_f32(const float* x, const float* w_packed, const float* bias, float* y, long long M, int C, int K,
                           int relu, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Winograd F(2x4,3x3) convolution, fp32 MFMA (csrc/seam_wino24.hip): the same layers and the same contract as
 * seam_conv3x3_wino_f32, with output tiles of 2 rows x 4 columns (F(2,3) down the rows, F(4,3) with the points
 * {0, +-1, +-2, inf} along the columns): 24 multiplies per 8 outputs -- 3x fewer matrix-core issues than
 * seam_conv2d_f32, 1.33x fewer than seam_conv3x3_wino_f32; rounding ~2x that of F(2x2,3x3) (~1e-6 of the output
 * scale).  u_packed: seam_wino24_weight_floats(K, Cstore) floats from seam_pack_conv_weight_wino24_f32 (U = G2 g G4t in
 * fp64, rounded once, MFMA fragment order).  seam_wino_issue_slots / seam_wino24_issue_slots: MFMA work of a launch
 * (block tile slots x positions) for the host's choice between the two forms (maps whose width is not a multiple of 4
 * can favour F(2x2)). */
long long seam_wino24_weight_floats(int K, int Cstore);
long long seam_wino24_issue_slots(int N, int H, int W, int C, int K, int pad);
int seam_wino24_variant(int N, int H, int W, int C, int K, int pad);   /* n-tiles per block (kernel variant conv3x3_wino24<NT>) picked for this shape; 0 = unsupported */
int seam_wino24_form(int N, int H, int W, int C, int K, int pad);      /* 1: the launch runs on the producer / consumer kernel conv3x3_wino24pc (round 5: the NT = 2 block as four MFMA-only waves + four transform / load waves, two per SIMD; bit-identical results), 0: conv3x3_wino24<NT>, -1: unsupported.  SEAM_W24_PC=0 in the environment keeps every launch on conv3x3_wino24<NT> */
long long seam_wino_issue_slots(int N, int H, int W, int C, int K, int pad);
int seam_pack_conv_weight_wino24_f32(const float* w, float* u_packed, int K, int Cin, int Cstore, int mode,
                                     seam_stream_t stream);
int seam_conv3x3_wino24_f32(const float* x, const float* u_packed, const float* scale, const float* shift,
                            const float* residual, float* y, int N, int H, int W, int C, int K, int pad, int relu,
                            seam_stream_t stream);

/* conv3x3_wino24sx (csrc/seam_wino24sx.hip): the same F(2x4,3x3) convolution with its 24 position GEMMs as six-term split-bf16
 * products on the bf16 matrix pipe -- V in fp32 by seam_conv3x3_wino24_f32's transform, cut into three bf16 pieces; U cut at pack
 * time from the fp32 value seam_pack_conv_weight_wino24_f32 writes; the products (2,0) (1,1) (0,2) (1,0) (0,1) (0,0) per k-step of 16
 * channels accumulated in fp32.  Results differ from seam_conv3x3_wino24_f32's in the last bits (measured against float64: within 3x
 * its error).  Shapes: C and K multiples of 64 from 64 on, stride 1, pad 0 | 1, any batch; _supported returns 1 for them, else 0, and
 * the launcher returns hipErrorInvalidValue with nothing launched.
 *   u_packed: seam_wino24sx_weight_bytes(K, Cstore) = 144 K Cstore bytes from seam_pack_conv_weight_wino24_sx
 *   ([K/32][Cstore/16][24 positions][3 planes][64 lanes][8 bf16]; mode as seam_pack_conv_weight_wino24_f32). */
long long seam_wino24sx_weight_bytes(int K, int Cstore);
int seam_pack_conv_weight_wino24_sx(const float* w, void* u_packed, int K, int Cin, int Cstore, int mode, seam_stream_t stream);
int seam_conv3x3_wino24sx_supported(int N, int H, int W, int C, int K, int pad, int stride);
long long seam_conv3x3_wino24sx_blocks(int N, int H, int W, int C, int K, int pad);   /* tiles of the launch (independent of the forced split); 0 = unsupported */
/* The XCD groups conv3x3_wino24sx splits its n-tiles over, process-wide: 0 (default) the launcher's rule, 1 | 2 | 4 | 8 forced (reduced
 * until it divides the n-tiles); set returns hipErrorInvalidValue for any other value and leaves the setting.  Same bits under every
 * value; for the parity test and the A/B tools. */
int seam_conv3x3_wino24sx_set_nsplit(int nsplit);
int seam_conv3x3_wino24sx_get_nsplit(void);
/* The block layout of a launch of the F(2x4) kernels, read from the arguments the launcher would launch with (host only, nothing is
 * launched): sx = 0 the plan of seam_conv3x3_wino24_f32, sx = 1 that of seam_conv3x3_wino24sx_f32 (two n-tiles per block, its own
 * acceptance rule, the currently forced split).  out[24], in this order: nreg (1..3 regions: main, right strip, bottom strip), stack
 * (1: TY[0] consecutive tile rows of the whole batch per block), G (images a block's patch spans), PH (patch rows, stacked form),
 * nt, tiles_n, nsplit, per_img (patch blocks of one image), TX[3], TY[3] (tiles per block patch; the kernel's LDS stride class is
 * HS = (TX + 1) | 1: 9, 5, 3 compiled, anything else the run-time form), bx[3], by[3] (blocks of a region), patch blocks (all
 * images, one n-tile), grid blocks (x n-tiles, plus the padding blocks of an n-tile split); out[22..23] = 0.  Regions past nreg
 * are 0.  Returns 0, or hipErrorInvalidValue with nothing written for a shape the launcher refuses. */
int seam_wino24_layout(int N, int H, int W, int C, int K, int pad, int sx, int* out);
int seam_conv3x3_wino24sx_f32(const float* x, const void* u_packed, const float* scale, const float* shift, const float* residual,
                              float* y, int N, int H, int W, int C, int K, int pad, int stride, int relu, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 3x3 / stride-1 convolution, fp16 operands / fp32 accumulation, producer / consumer form (csrc/seam_f16pc.hip, round 5): the
 * config-5 path's 3x3 layers (ResNet / FPN / RPN / mask head / match trunk; ref models/video_matchrcnn.py:337-338,
 * models/match_head.py:50-58) with the input patch staged in LDS once per 64-channel chunk instead of gathered nine times.  Same
 * contract as seam_conv2d_f16 on those shapes (NHWC fp16 in / out, per-channel fp32 scale / shift, ReLU) except that a residual
 * operand is NOT taken (`residual` must be NULL, else hipErrorInvalidValue: no 3x3 layer of the path has one, and the kernel's
 * epilogue rounds to fp16 in the accumulator registers); fp32 accumulation in a different order than seam_conv2d_f16 (chunk-major
 * instead of tap-major): results agree to fp32 rounding of the accumulation, not bit for bit.  Weights:
 * seam_f16pc_weight_halves(K, Cstore) fp16 values from seam_pack_conv_weight_f16pc (OIHW fp32 in; MFMA fragment order).  Shapes:
 * seam_conv3x3_f16pc_supported (C a multiple of 128, K a multiple of 128, pad 0 | 1; maps of >= 24 output columns or whole maps
 * of <= 16 x 16 outputs); seam_conv3x3_f16pc_pays = supported AND expected faster than seam_conv2d_f16 (tiles >= 3/4 full; a
 * function of the map geometry only, not of N) -- the rule the host side dispatches by. */
int seam_conv3x3_f16pc_supported(int N, int H, int W, int C, int K, int pad);
int seam_conv3x3_f16pc_pays(int N, int H, int W, int C, int K, int pad);
long long seam_f16pc_weight_halves(int K, int Cstore);
int seam_pack_conv_weight_f16pc(const float* w, void* w_packed, int K, int Cin, int Cstore, seam_stream_t stream);
int seam_conv3x3_f16pc(const void* x, const void* w_packed, const float* scale, const float* shift, const void* residual, void* y,
                       int N, int H, int W, int C, int K, int pad, int relu, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The match trunk as one call (SURVEY.md 8b `seam_match_trunk_f32`): MatchPredictor / TemporalAggregationNLB's
 * conv_seq (4 valid 3x3 convs + ReLU, 14 -> 12 -> 10 -> 8 -> 6) -> AvgPool2d(6,6) + ReLU -> Linear(1024,256) + BatchNorm1d
 * (ref models/match_head.py:50-62,67-69,93-95).  roi NHWC [K,14,14,256] -> x3 [K,256].  Six launches on `stream` (why the
 * kernels are not fused further: csrc/seam_trunk.hip).  conv[4] / linear: the packed weights of the layers -- `w` from
 * seam_pack_conv_weight_f32 (required for `linear`; for a conv it may be NULL when a Winograd form is given), `u` / `u24` from
 * seam_pack_conv_weight_wino_f32 / _wino24_f32 or NULL, `scale` / `shift` the [K] epilogue vectors (bias; for `linear` the folded
 * BatchNorm1d) or NULL.  form: int[4] per conv -- 0 implicit GEMM, 1 F(2x2,3x3), 2 F(2x4,3x3) -- or NULL: chosen on the map
 * geometry as the Python layer does.  ws: >= seam_match_trunk_workspace_floats(K) floats. */
typedef struct {
    const float* w;
    const float* u;
    const float* u24;
    const float* scale;
    const float* shift;
} seam_trunk_layer_t;
int64_t seam_match_trunk_workspace_floats(int K);
int seam_match_trunk_f32(const float* roi, const seam_trunk_layer_t* conv, const seam_trunk_layer_t* linear, float* x3,
                         int K, float* ws, const int* form, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Gradient kernels of the match heads: the grad-enabled pass of the training loop,
 * stuffs/engine.py:120-121,158-168,183-185 -> MatchPredictor / TemporalAggregationNLB in .train()
 * (models/match_head.py:66-76,90-169,339).  fp32, fixed-order reductions (bit-reproducible).
 *
 * seam_conv_wgrad_f32: dw [K,C,R,S] (OIHW) = sum_{n,ho,wo} dy[n,ho,wo,k] * x[n,ho*stride+r-pad,wo*stride+s-pad,c]
 *   for x NHWC [N,H,W,C], dy NHWC [N,Ho,Wo,K]; C,K multiples of 4.  fp32-MFMA GEMM split over the pixel
 *   axis; ws: >= seam_conv_wgrad_workspace_floats(M = N*Ho*Wo, C, K, R, S) floats.  (Linear: R=S=1, H=W=1.)
 *   Refused (non-zero return, nothing launched or written): N <= 0, Ho <= 0, Wo <= 0, C % 4, K % 4, and either
 *   operand of 2^31 bytes or more -- M*K*4 >= 2^31 (dy) or N*H*W*C*4 >= 2^31 (x): the kernel's buffer offsets are 32-bit.
 * seam_conv_wgrad_crop_f32: the same sum for a conv whose output was cropped to its first Ho x Wo positions (the stem on the
 *   space-to-depth frame: 4x4 / stride 1 / pad 2 cropped to the input grid): dy NHWC [N,Ho,Wo,K] is read as it lies, no copy
 *   onto the conv's own grid.  ws for M = N*Ho*Wo.  Refused as above, and: Ho or Wo beyond the conv's own output grid,
 *   R, S, stride, H, W <= 0, pad < 0, a NULL pointer.
 * seam_colsum_f32: out[k] = sum_m x[m,k]  (bias gradients); ws: >= seam_colsum_workspace_floats(M,K) floats.
 *   M = 0 writes zeros; K <= 0 returns 0 and writes nothing. */
int64_t seam_conv_wgrad_workspace_floats(int M, int C, int K, int R, int S);
int seam_conv_wgrad_f32(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K,
                        int R, int S, int stride, int pad, float* ws, seam_stream_t stream);
int seam_conv_wgrad_crop_f32(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K,
                             int R, int S, int stride, int pad, int Ho, int Wo, float* ws, seam_stream_t stream);
int64_t seam_colsum_workspace_floats(int M, int K);
int seam_colsum_f32(const float* x, float* out, int M, int K, float* ws, seam_stream_t stream);

/* Backward of conv_seq's last ReLU -> AvgPool2d(6,6) -> ReLU (models/match_head.py:56-60):
 * dy[n,hw,c] = y[n,hw,c] > 0 ? dpool[n,c] / HW : 0   (y = the ReLU'd conv output, NHWC [N,HW,C]; a correctly
 * rounded division).  N*HW*C == 0 returns 0 and writes nothing. */
int seam_avgpool_relu_bwd_f32(const float* dpool, const float* y, float* dy, int N, int HW, int C,
                              seam_stream_t stream);

/* nn.BatchNorm1d(256) in training mode (models/match_head.py:62): batch statistics over the M rows (M >= 2),
 * running_mean/var updated in place with `momentum` (unbiased variance), or left alone when NULL;
 * save_mean / save_invstd [F] feed seam_bn1d_bwd_f32 (dx, dgamma, dbeta).  The statistics are shifted, corrected
 * two-pass sums (their error scales with a column's spread, not its offset).
 * Refused (nothing written): the forward when M < 2 or F <= 0 (torch: "Expected more than 1 value per channel when
 * training"), the backward when M <= 0 or F <= 0. */
int seam_bn1d_train_fwd_f32(const float* x, const float* gamma, const float* beta, float* y,
                            float* save_mean, float* save_invstd, float* running_mean,
                            float* running_var, int M, int F, float momentum, float eps,
                            seam_stream_t stream);
int seam_bn1d_bwd_f32(const float* dy, const float* x, const float* save_mean, const float* save_invstd,
                      const float* gamma, float* dx, float* dgamma, float* dbeta, int M, int F,
                      int frozen /* 1: eval-mode statistics, dx = gamma*invstd*dy */, seam_stream_t stream);

/* nn.CrossEntropyLoss(weight=[w0,w1]) over [n,2] logits with int64 targets, mean reduction -- the criterion of
 * every loss of models/match_head.py (:213,257,367,386): loss [1] and dloss/dlogits [n,2] in one launch.
 * n <= 0 is refused (nothing written).  If the weights of the targets' classes sum to 0, loss and dlogits are NaN (0/0),
 * as in torch. */
int seam_ce2_fwd_bwd_f32(const float* logits, const int64_t* target, const float* weight, float* loss,
                         float* dlogits, int64_t n, seam_stream_t stream);

/* Gradients of seam_pair_logits_f32: g [Q,G,2] -> da [Q,256], db [G,256], dw [2,256], dbias [2].
 * Refused (nothing written): D != 256, Q <= 0, G <= 0. */
int seam_pair_logits_bwd_f32(const float* a, const float* b, const float* w, const float* g, float* da,
                             float* db, float* dw, float* dbias, int Q, int G, int D,
                             seam_stream_t stream);

/* Gradients of seam_nlb_attnpool_f32 (same operand layouts; Tmax <= 64): dout [S,256] -> dseq (same strides
 * as seq; only rows t < len[s] are written) and the parameter gradients, grads[11] = device pointers in the
 * reference's layouts: theta.weight [128,256], theta.bias [128], phi.weight, phi.bias, g.weight, g.bias,
 * concat_project.0.weight [256], W.weight [256,128], W.bias [256], attention_scorer.weight [256], .bias [1].
 * ws: >= seam_nlb_bwd_workspace_floats(S,Tmax) floats.  len[s] > Tmax is read as Tmax, len[s] <= 0 as an empty sequence
 * (no row written).  Refused (nothing written): Tmax > 64 (a sequence is kept in LDS) or Tmax <= 0; S <= 0 returns 0. */
int64_t seam_nlb_bwd_workspace_floats(int S, int Tmax);
int seam_nlb_attnpool_bwd_f32(const float* seq, int64_t t_stride, int64_t s_stride, const int* len, int S,
                              int Tmax, const float* w_proj_t, const float* b_proj, const float* w_cat,
                              const float* w_out_t, const float* b_out, const float* w_att,
                              const float* b_att, const float* dout, float* dseq, float* const* grads,
                              float* ws, int use_nlb, seam_stream_t stream);

/* Gradients of the non-local block ALONE -- the z output of seam_nlb_attnpool_f32, i.e. NONLocalBlock1D.forward called
 * directly and grad-enabled (ref models/nlb.py:66-101): dz rows at dz + s*dz_s_stride + t*dz_t_stride (256 floats each)
 * -> dseq (as above) and grads[9] = the first nine pointers of the list above (no attention scorer behind a direct call).
 * Same workspace, length rules and refusals as seam_nlb_attnpool_bwd_f32, and dz == NULL is refused. */
int seam_nlb_block_bwd_f32(const float* seq, int64_t t_stride, int64_t s_stride, const int* len, int S, int Tmax,
                           const float* w_proj_t, const float* b_proj, const float* w_cat,
                           const float* w_out_t, const float* b_out, const float* dz, int64_t dz_t_stride,
                           int64_t dz_s_stride, float* dseq, float* const* grads, float* ws, int use_nlb,
                           seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Input pipeline on the device: what MovingFashionDataset.__getitem__ does to a decoded
 * frame (datasets/MFDataset.py:79-93), on uint8 [H,W,3] device images.
 *
 * seam_frame_noise_u8: rgb = uint8(clip((bgr[...,::-1] / 255.0 + n * sigma) * 255.0, 0, 255)), float64 like NumPy;
 *   n = noise[H,W,3] float64 standard-normal draws, or (noise NULL) counter-based draws keyed by `seed`;
 *   sigma 0 with noise NULL = the noise=False branch (channel flip only).
 * seam_resize_bicubic_u8: PIL Image.resize((OW,OH)) -- BICUBIC, antialiased, 8-bit fixed point, horizontal then
 *   vertical pass -- bit-identical to Pillow (MFDataset.py:92: half resolution); ws: seam_resize_workspace_bytes. */
int seam_frame_noise_u8(const uint8_t* bgr, const double* noise, uint8_t* rgb, int H, int W, double sigma,
                        uint64_t seed, seam_stream_t stream);
/* seam_noise_u8_batch: the noise of MultiDeepFashion2Dataset.__getitem__ (datasets/MultiDF2Dataset.py:157-167) for a whole batch
 *   of uint8 HWC RGB images of different sizes, in place in the flat DEVICE buffer `buf` that seam_preprocess_u8_batch_f32 reads
 *   (img_off int64 [n_images] byte offsets, img_dims int32 [n_images,5] of which in_h and in_w are read), ONE launch:
 *   byte e of image i becomes uint8(clip((v / 255.0 + n * sigma[i]) * 255.0, 0, 255)) in float64, n = draws[draws_off[i] + e]
 *   (float64 draws, element offsets) or, draws NULL, the counter-based draw seam_frame_noise_u8 makes for (seed[i], e).  Element
 *   order is the image's own (unflipped).  An image with sigma 0, or whose in_h * in_w * 3 bytes at img_off do not lie inside
 *   buf_bytes, is left as it is; nothing outside an image is written. */
int seam_noise_u8_batch(uint8_t* buf, int64_t buf_bytes, const int64_t* img_off, const int* img_dims, const double* sigma,
                        const uint64_t* seed, const double* draws, const int64_t* draws_off, int n_images,
                        seam_stream_t stream);
/* seam_frames_prepare_batch_u8: the per-frame work of MovingFashionDataset.__getitem__ (datasets/MFDataset.py:79-95) for a whole
 *   batch of uint8 HWC images of different sizes, ONE launch.  Image i lies at byte in_off[i] of the flat DEVICE buffer `in`
 *   (in_off int64 [n_images]; dims int32 [n_images,3] = (h, w, mode)) and its result is written at byte out_off[i] of `out`:
 *     mode 0  the bytes as they are (the RGB shop image, the zero placeholder of an unreadable frame), h x w;
 *     mode 1  BGR -> RGB (the dataset's noise=False branch), h x w;
 *     mode 2  BGR -> RGB, the noise of seam_frame_noise_u8 (sigma[i]; n = draws[draws_off[i] + e], float64 draws at element
 *             offsets, draws_len of them in all, or, draws NULL, the counter-based draw for (seed[i], e), e the element index
 *             in the full-resolution RGB frame), then seam_resize_bicubic_u8 to (h / 2) x (w / 2), fused: no intermediate
 *             image is written.  Bit-identical to seam_frame_noise_u8 + seam_resize_bicubic_u8 for h, w >= 2.
 *   max_h / max_w: the largest h and w of the batch (the sizes themselves are on the device; they size the grid).  An image
 *   whose input or output bytes do not lie inside in_bytes / out_bytes, whose draws do not lie inside draws_len, whose mode is
 *   not 0..2, that exceeds max_h / max_w or (mode 2) has h or w < 2 is skipped: nothing of it is read or written.  `in` and
 *   `out` must not overlap, nor the outputs of two images.  The output buffer is in the layout seam_preprocess_u8_batch_f32
 *   reads, with out_off as its img_off. */
int seam_frames_prepare_batch_u8(const uint8_t* in, int64_t in_bytes, const int64_t* in_off, const int* dims,
                                 const double* sigma, const uint64_t* seed, const double* draws, const int64_t* draws_off,
                                 int64_t draws_len, uint8_t* out, int64_t out_bytes, const int64_t* out_off, int n_images,
                                 int max_h, int max_w, seam_stream_t stream);
int64_t seam_resize_workspace_bytes(int H, int W, int OH, int OW);
int seam_resize_bicubic_u8(const uint8_t* in, uint8_t* out, int H, int W, int OH, int OW, void* ws,
                           seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training branch of the RoI heads (ref models/matchrcnn.py:333-472, torchvision roi_heads [TV]), csrc/seam_roi_train.hip.
 * Every kernel reduces in a fixed order: a launch is bit-identical to the next.
 *
 * seam_roi_sample_f32: select_training_samples per image, one workgroup each.  cand [N,P,4] xyxy (the image's proposals
 *   followed by its GT boxes; n_cand[i] <= P rows are real), keys [N,P] (one uniform draw per candidate), gt_boxes [N,G,4],
 *   gt_labels int64 [N,G] (n_gt[i] rows real).  Matcher(0.5, 0.5) on box_iou in fp32 (first GT on ties; background label
 *   0, matched index 0); BalancedPositiveNegativeSampler(batch, pos_max / batch): the min(#pos, pos_max) positives
 *   (label >= 1) and min(#neg, batch - that) negatives (label 0) with the smallest (key, index); the sampled rows in
 *   ascending candidate order -> idx, labels, matched (int64 [N,batch]), boxes and BoxCoder((wx,wy,ww,wh)).encode targets
 *   ([N,batch,4]); rows past the count: idx/labels/matched -1, boxes/targets 0.  count int32 [N,2] = (rows, positives),
 *   (-1,-1) for an image with no GT box.  Refused: P outside 1..16384, G outside 1..32767, batch outside 1..16384,
 *   pos_max outside 0..batch, a NULL pointer.
 * seam_fastrcnn_loss_fwd_bwd_f32: fastrcnn_loss [TV] on R rows: loss[0] = mean cross entropy of class_logits [R,ncls]
 *   against labels int64 [R]; loss[1] = smooth-L1 (beta 1/9) of box_regression [R,4*ncls] at the label's 4 deltas
 *   against targets [R,4], summed over the rows with label > 0, / R; dclass, dbox = their gradients (for a unit upstream
 *   gradient; zeros outside the label's deltas).  A label outside 0..ncls-1 makes both losses NaN.  One workgroup.
 * seam_mask_loss_fwd_bwd_f32: maskrcnn_loss [TV] on P positive ROIs: logits [P,14,14,4,ncls] (the sub-pixel layout of
 *   MaskRCNNPredictor), labels int64 [P], rois [P,4] xyxy in the masks' frame; ROI k's GT mask is the uint8 [H,W] map at
 *   masks + mask_off[k] with (H,W) = mask_hw[2k..2k+1].  Target = roi_align(mask, roi, 28, 1.0, sampling_ratio=-1,
 *   aligned=False), recomputed per bin and never stored; loss = mean BCE-with-logits on the label channel;
 *   dlogits (layout of logits) = its gradient, zeros in the other channels.  ws: P floats.  Refused: P outside
 *   1..21399 (P*784 < 2^24), ncls outside 1..65536, a NULL pointer. */
int seam_roi_sample_f32(const float* cand, const int* n_cand, const float* keys, const float* gt_boxes, const int64_t* gt_labels,
                        const int* n_gt, int N, int P, int G, int batch, int pos_max, float wx, float wy, float ww, float wh,
                        int64_t* idx, int64_t* labels, int64_t* matched, float* boxes, float* targets, int* count,
                        seam_stream_t stream);
int seam_fastrcnn_loss_fwd_bwd_f32(const float* class_logits, const float* box_regression, const int64_t* labels,
                                   const float* targets, int R, int ncls, float* loss, float* dclass, float* dbox,
                                   seam_stream_t stream);
int seam_mask_loss_fwd_bwd_f32(const float* logits, const int64_t* labels, const float* rois, const uint8_t* masks,
                               const int64_t* mask_off, const int* mask_hw, int P, int ncls, float* loss, float* dlogits,
                               float* ws, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training branch of the RPN (torchvision RegionProposalNetwork.assign_targets_to_anchors / compute_loss [TV]),
 * csrc/seam_rpn_train.hip.  Sized for 2^20 anchors per image: many workgroups per image, state in the caller's workspace.
 * Float reductions run in a fixed order and the only atomics are integer ones: a launch is bit-identical to the next.
 * Caps (a call outside them is refused and writes nothing): N 1..4096 images, A 1..2^20 anchors, G 1..seam_rpn_max_gt() = 128
 * GT boxes per image, batch 1..1024.
 *
 * seam_rpn_match_f32: Matcher(fg_thresh, bg_thresh, allow_low_quality_matches=True) of anchors [A,4] (shared by the batch)
 *   against gt_boxes [N,G,4] (n_gt[i] rows real; boxes must be finite), box_iou in fp32 in torchvision's expression order.
 *   Per anchor the maximum over the GT boxes (first GT on ties): < bg_thresh -> label 0, < fg_thresh -> label -1 (ignored),
 *   else label 1.  Low-quality rule: every anchor whose IoU with some GT box EQUALS that box's largest IoU over the image's
 *   anchors becomes foreground, matched to its own argmax GT (a GT box that overlaps no anchor has maximum 0, which every
 *   anchor equals: the whole image turns foreground, as in torchvision).  n_gt[i] == 0: all background.
 *   labels int8 [N,A]; matched int32 [N,A] = the argmax GT of a foreground anchor, 0 otherwise.
 *   ws: seam_rpn_match_workspace_floats(N, A, G) floats (0 = outside the caps).  Also refused: bg_thresh > fg_thresh, NULL.
 * seam_rpn_sample_f32: BalancedPositiveNegativeSampler(batch, pos_max / batch) on those labels with one uniform key per
 *   anchor (keys [N,A]): the min(#foreground, pos_max) foreground and min(#background, batch - that) background anchors
 *   with the smallest (key, index), by a radix select over ord(key) << 20 | index in global memory.  idx int64 [N,batch]:
 *   the sampled anchors in ascending order, -1 past the count; slabels (1 / 0; -1 past the count) and smatched int64
 *   [N,batch]; targets [N,batch,4] = BoxCoder((1,1,1,1)).encode(matched GT, anchor) on the foreground rows, 0 elsewhere;
 *   count int32 [N,2] = (rows, foreground rows).  ws: seam_rpn_sample_workspace_bytes(N, batch) bytes.
 *   Also refused: pos_max outside 0..batch, NULL.
 * seam_rpn_gather_patches_f32: the 3x3 input window of the RPN conv at M sampled pixels.  maps: HOST array of L device
 *   pointers to NHWC fp32 maps [N,H_l,W_l,C]; hw: HOST array of 2L ints (H_l, W_l); rows: device int32 [M,4] =
 *   (image, level, y, x) -> out [M,3,3,C], zeros outside the map (the conv's padding) and for a row whose image, level or
 *   pixel is out of range.  Refused: M outside 1..2^20, L outside 1..8, C outside 4..4096 or not a multiple of 4, NULL.
 * seam_rpn_loss_fwd_bwd_f32: compute_loss on the M sampled rows.  head [M,head_cols]: the head's outputs at each row's
 *   pixel (A objectness logits, then 4A deltas); slot int32 [M]: the row's anchor slot a; labels int64 [M] (1 / 0);
 *   targets [M,4].  loss[0] = mean BCE-with-logits(head[r,a], label); loss[1] = smooth-L1 (beta 1/9) of
 *   head[r, A+4a..A+4a+3] against targets on the label-1 rows, summed, / M.  grad [M,grad_cols] = both gradients for a
 *   unit upstream gradient, zeros elsewhere (grad_cols >= 5A: the padding the input-gradient conv wants).  A slot outside
 *   0..A-1 or a label outside {0,1} makes both losses NaN.  One workgroup.  Refused: M outside 1..2^20, A outside 1..64,
 *   head_cols or grad_cols outside 5A..1024, NULL. */
int seam_rpn_max_gt(void);
int64_t seam_rpn_match_workspace_floats(int N, int A, int G);
int seam_rpn_match_f32(const float* anchors, const float* gt_boxes, const int* n_gt, int N, int A, int G, float fg_thresh,
                       float bg_thresh, int8_t* labels, int* matched, float* ws, seam_stream_t stream);
int64_t seam_rpn_sample_workspace_bytes(int N, int batch);
int seam_rpn_sample_f32(const int8_t* labels, const int* matched, const float* keys, const float* anchors, const float* gt_boxes,
                        int N, int A, int G, int batch, int pos_max, int64_t* idx, int64_t* slabels, int64_t* smatched,
                        float* targets, int* count, void* ws, seam_stream_t stream);
int seam_rpn_gather_patches_f32(const void* const* maps, const int* hw, const int* rows, int M, int N, int L, int C, float* out,
                                seam_stream_t stream);
int seam_rpn_loss_fwd_bwd_f32(const float* head, const int* slot, const int64_t* labels, const float* targets, int M, int A,
                              int head_cols, int grad_cols, float* loss, float* grad, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training the FPN (torchvision FeaturePyramidNetwork under the heads' six losses), csrc/seam_fpn_train.hip: the adjoints of
 * RoIAlign, of the RPN's 3x3-window gather and of the nearest top-down merge.  The dense convolutions of the FPN backward
 * run on seam_conv2d_f32 over rotated weights, seam_conv_wgrad_f32 and seam_colsum_f32.  fp32, NHWC.
 * No float atomics: every output element is summed by one thread in a fixed order, so a launch is bit-identical to the
 * next, and every entry point writes its outputs completely (zeros where nothing arrives).
 *
 * seam_roi_align_bwd_f32: adjoint of seam_roi_align_f32 -- same rois [K,5], levels (or NULL: the forward's LevelMapper, one
 *   shared device function, so a ROI on a level boundary sends its gradient to the level the forward read), hw, C, scales,
 *   k_min, P, sampling_ratio; dout NHWC [K,P,P,C] -> the four gradient maps dfeat_l [N,H_l,W_l,C], written completely
 *   (whole images that own no ROI are zeros; K == 0 writes zeros and needs no rois / dout).  torchvision
 *   roi_align(aligned=False) backward: samples with a coordinate < -1 or > size contribute nothing, coordinates clamped at
 *   0, last row / column collapse, ROI extent >= 1, bin average / sr^2.  The sample positions are torchvision's fp32
 *   operation sequence with no fused multiply-add (the forward kernel fuses one, which can move a position by an ulp).
 *   A ROI whose image index is outside [0,N) or not finite, or whose given level is outside 0..3, contributes nothing; no
 *   ROI can cause an access outside the maps (gather form: a workgroup writes only its own 8x8-pixel tile).
 *   ws: seam_roi_align_bwd_workspace_bytes(N, K) bytes (0 = outside the caps).
 *   Refused, nothing launched or written: C % 4, C outside 4..4096, P outside 1..32, sampling_ratio outside 1..64, N outside
 *   1..4096, K outside 0..2^20, a NULL pointer, a map extent <= 0, a map of 2^31 bytes or more.
 * seam_rpn_scatter_patches_f32: adjoint of seam_rpn_gather_patches_f32 -- dpatch [M,3,3,C], rows int32 [M,4] = (image, level,
 *   y, x), dmaps / hw HOST arrays as in the gather: dmap_l[n, y+r-1, x+s-1, :] += dpatch[m,r,s,:] for the taps inside the
 *   map, in row order; the maps are written completely (zeros elsewhere); a row whose image, level or pixel is out of range
 *   contributes nothing.  Caps and refusals of the gather (M 1..2^20, L 1..8, C 4..4096 % 4, NULL), and N 1..4096.
 * seam_upsample_add_bwd_f32: adjoint of seam_upsample_add_f32 / seam_conv2d_upres_f32 (one shared index function):
 *   dtop[n,ht,wt,:] = base[n,ht,wt,:] + sum of dlat[n,h,w,:] over the fine pixels the forward maps to (ht,wt), rows then
 *   columns ascending; base may be NULL, and may be dtop itself.  dlat [N,H,W,C], dtop / base [N,Ht,Wt,C]; any size ratio.
 * seam_subsample_add_bwd_f32: adjoint of LastLevelMaxPool (max_pool2d k=1, s=2): d[n,2i,2j,:] += dpool[n,i,j,:] in place;
 *   d [N,H,W,C], dpool [N,Hp,Wp,C] with Hp = (H-1)/2+1, Wp = (W-1)/2+1 (anything else is refused).
 * The last two refuse a non-positive extent, C % 4 and a NULL pointer. */
int64_t seam_roi_align_bwd_workspace_bytes(int N, int K);
int seam_roi_align_bwd_f32(const float* dout, const float* rois, const int* levels, const int* hw, int C, float scale0,
                           float scale1, float scale2, float scale3, int k_min, int N, int K, int P, int sampling_ratio,
                           float* dfeat0, float* dfeat1, float* dfeat2, float* dfeat3, void* ws, seam_stream_t stream);
int seam_rpn_scatter_patches_f32(const float* dpatch, const int* rows, int M, int N, int L, int C, void* const* dmaps,
                                 const int* hw, seam_stream_t stream);
int seam_upsample_add_bwd_f32(const float* dlat, const float* base, float* dtop, int N, int H, int W, int Ht, int Wt, int C,
                              seam_stream_t stream);
int seam_subsample_add_bwd_f32(float* d, const float* dpool, int N, int H, int W, int Hp, int Wp, int C, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training the ResNet body (torchvision Bottleneck v1.5 with FrozenBatchNorm2d), csrc/seam_body_train.hip.  The stride-1
 * convolutions of the bottleneck backward run on seam_conv2d_f32 / the Winograd kernels over rotated weights and on
 * seam_conv_wgrad_f32; the 1x1 / stride-2 shortcut adjoint is seam_subsample_add_bwd_f32.  What is added here: the input
 * gradient of the three 3x3 / stride-2 / pad-1 convs (layer{2,3,4}.0.conv2) and the ReLU at a block's output.  fp32, NHWC,
 * no float atomics, a fixed summation order (two launches give the same bits), every output element written exactly once.
 *
 * seam_conv3x3s2_dgrad_f32: dy NHWC [N,Ho,Wo,K] with Ho = (H-1)/2+1, Wo = (W-1)/2+1; the forward conv's OIHW weight
 *   w [K,C,3,3] and the FrozenBN scale [K] (or NULL) of its epilogue packed by seam_pack_conv3x3s2_dgrad_f32 into
 *   w_packed [9][C][K] (9*C*K floats, w_packed[r*3+s][c][k] = scale[k] * w[k,c,r,s]: dy*scale is never materialised);
 *   mask NHWC [N,H,W,C] or NULL; dx NHWC [N,H,W,C]:
 *     dx[n,h,w,c] = sum over (r,s,ho,wo) with 2*ho+r-1 == h, 2*wo+s-1 == w, 0<=ho<Ho, 0<=wo<Wo of
 *                   scale[k] * dy[n,ho,wo,k] * w[k,c,r,s], summed over k;   dx = 0 where mask <= 0.
 *   A gather: an even row has the tap r = 1 (ho = h/2), an odd row r = 0 (ho = (h+1)/2) and r = 2 (ho = (h-1)/2), columns
 *   alike, so the four (row parity, column parity) classes of input pixels are GEMMs over 1, 2, 2 and 4 taps -- 9/4 taps
 *   per pixel, one launch, v_mfma_f32_32x32x2_f32.  Taps with ho == Ho or wo == Wo (last odd row / column of an even-sized
 *   map) do not exist and contribute nothing.
 *   Refused, nothing launched or written: N, H, W <= 0, C % 32, K % 32, a NULL dy / w_packed / dx, dy or dx of 2^31 bytes or more
 *   (split the batch over images).  The pack refuses K % 32, C % 32 and a NULL w / w_packed.
 * seam_relu_mask_add_f32: out[m,c] = y[m,c] > 0 ? a[m,c] + b[m,c] : 0 over [M,C], b NULL or a second gradient; 16 bytes per
 *   lane.  Refused: M <= 0, C <= 0, C % 4, a NULL y / a / out.
 * seam_maxpool3s2_relu_bwd_f32: the adjoint of the stem's max-pool (3x3 / stride 2 / pad 1) fused with the stem's ReLU mask.
 *   y NHWC [N,H,W,C] is the pool's input (the stem output after FrozenBN + ReLU; finite), dpool NHWC [N,Ho,Wo,C] with
 *   Ho = (H-1)/2+1, Wo = (W-1)/2+1 the gradient of the pooled map, dy NHWC [N,H,W,C]:
 *     dy[n,h,w,c] = y[n,h,w,c] > 0 ? sum over the windows (ph,pw), |2ph-h| <= 1, |2pw-w| <= 1, 0 <= ph < Ho, 0 <= pw < Wo, whose
 *                   argmax is (h,w), of dpool[n,ph,pw,c] : 0      (1, 2 or 4 windows, added in ascending (ph,pw) order)
 *   The argmax of a window is torch's: the first maximum in row-major order of its cells inside the image (strict > to replace).
 *   A gather: a lane owns the pixels (2a+{0,1}, 2b+{0,1}) of four channels, which lie in the windows (a+{0,1}, b+{0,1}) only;
 *   16 bytes per lane along C, every dy element written exactly once.
 *   Refused, nothing launched or written: N, H, W, C <= 0, C % 4, a NULL pointer, y of 2^31 bytes or more. */
int seam_pack_conv3x3s2_dgrad_f32(const float* w, const float* scale, float* w_packed, int K, int C, seam_stream_t stream);
int seam_conv3x3s2_dgrad_f32(const float* dy, const float* w_packed, const float* mask, float* dx, int N, int H, int W, int C, int K,
                             seam_stream_t stream);
int seam_relu_mask_add_f32(const float* y, const float* a, const float* b, float* out, int64_t M, int C, seam_stream_t stream);
int seam_maxpool3s2_relu_bwd_f32(const float* y, const float* dpool, float* dy, int N, int H, int W, int C, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Ground-truth masks from annotations, csrc/seam_masks.hip: COCO-style polygon lists and RLE counts rasterised into the
 * uint8 0/1 [n,H,W] stacks that the mask loss and the segm AP read (ref datasets/DF2Dataset.py:152-155: annToMask on the CPU,
 * then n*H*W bytes over the bus).  One call serves a batch of n objects from images of different sizes; object o's [h,w]
 * bytes go to out + obj_out_off[o] (int64 byte offsets), obj_hw int32 [n][2] = (h, w), 1 <= h, w <= 16384.  Every byte of
 * every object is written (nothing relies on a zeroed `out`); nothing is allocated, nothing synchronises.  The arithmetic
 * restates maskApi.c's rleFrPoly / rleMerge / rleDecode (float64, multiply and add kept apart); two calls give the same bits.
 * Not pinned against pycocotools itself.
 *
 * seam_poly_masks_u8: P polygon parts with V vertices in all.  pts int32 [V][2]: the vertices upsampled by 5 on the host,
 *   (int)(5*x + 0.5), (int)(5*y + 0.5), the ring NOT closed; part_off int32 [P+1]: CSR of the parts over the vertices;
 *   part_obj int32 [P]: each part's object, non-decreasing (an object's parts are adjacent; an object without parts is zeros);
 *   edge_pt_off int32 [V+1]: running sum of max(|dx|,|dy|) + 1 over the ring edges (vertex e -> vertex e+1, a part's last
 *   vertex back to its first), T = edge_pt_off[V] < 2^31 points in all; part_ws_off int64 [P+1]: running sum, in 32-bit words,
 *   of seam_poly_masks_ws_bytes(h, w) / 4 over the parts; ws: ws_bytes = 4 * part_ws_off[P] bytes, cleared by the call.
 *   An object is the union of its parts.  All tables are DEVICE arrays.
 * seam_poly_masks_ws_bytes: bytes of one part's bitmap on an h x w image, 4 * w * ceil((h+1)/32); 0 for a size out of range.
 * seam_rle_masks_u8: run_start int32: per object the exclusive running sum of its RLE counts (column-major runs of 0 and 1
 *   alternating, the first a run of zeros; a zero-length run repeats a start); obj_run_off int32 [n+1]: CSR of the objects over
 *   the runs.  A pixel's value is (index of the last run starting at or before its column-major position) & 1.
 * Refused, nothing launched or written: a negative count, a NULL table that the counts make necessary, ws_bytes % 4. */
int64_t seam_poly_masks_ws_bytes(int h, int w);
int seam_poly_masks_u8(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                       const int64_t* part_ws_off, const int* obj_hw, const int64_t* obj_out_off, uint8_t* out, void* ws,
                       int64_t ws_bytes, int P, int V, int T, int n, seam_stream_t stream);
int seam_rle_masks_u8(const int* run_start, const int* obj_run_off, const int* obj_hw, const int64_t* obj_out_off,
                      uint8_t* out, int n, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The input stage of a training step, csrc/seam_input.hip: a batch that crossed the bus as image bytes and annotation integers.
 *
 * seam_preprocess_u8_batch_f32: n uint8 HWC RGB images of different sizes in one flat DEVICE buffer `imgs` of imgs_bytes bytes,
 *   image i at byte img_off[i] (int64 [n], any alignment), img_dims int32 [n][5] = (in_h, in_w, out_h, out_w, flip).  ONE launch:
 *   ToTensor (byte / 255.f) + horizontal flip + (v - mean) / std + bilinear resize to (out_h, out_w) + zero pad to (Hp, Wp) +
 *   layout: s2d = 0 -> out [n, Hp, Wp, 4] (fourth channel zero), s2d != 0 -> out [n, Hp/2, Wp/2, 12], channel (dy*2 + dx)*3 + c
 *   = pixel (2Y+dy, 2X+dx), colour c.  Every cell of `out` is written (zero outside an image's out_h x out_w).  The arithmetic is
 *   seam_preprocess_f32 / seam_preprocess_s2d_batch_f32 on the flipped byte / 255.f image, bit for bit.  An image whose entry
 *   does not fit imgs_bytes or the padded frame is written as zeros.
 *   Refused: n < 1, n > 65535, Hp or Wp < 1, Hp > 65535, odd Hp / Wp with s2d, a NULL pointer.
 * seam_poly_masks_resized_u8 / seam_rle_masks_resized_u8: the tables of seam_poly_masks_u8 / seam_rle_masks_u8 (obj_hw is the
 *   SOURCE image size) plus obj_out int32 [n][3] = (out_h, out_w, flip); object o's [out_h, out_w] bytes go to
 *   out + obj_out_off[o], output pixel (r, c) = source pixel (sy(r), flip ? w - 1 - sx(c) : sx(c)), s(i) = min(floor(i *
 *   ((float)in / (float)out)), in - 1) in fp32 (ATen's nearest rule): the nearest resize of the flipped mask, without the
 *   original-size stack.  An object reaching past out_bytes is skipped.  Same toggle + scan stages, same refusals. */
int seam_preprocess_u8_batch_f32(const uint8_t* imgs, int64_t imgs_bytes, const int64_t* img_off, const int* img_dims, float* out,
                                 int n, int Hp, int Wp, int s2d, seam_stream_t stream);
int seam_poly_masks_resized_u8(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                               const int64_t* part_ws_off, const int* obj_hw, const int* obj_out, const int64_t* obj_out_off,
                               uint8_t* out, int64_t out_bytes, void* ws, int64_t ws_bytes, int P, int V, int T, int n,
                               seam_stream_t stream);
int seam_rle_masks_resized_u8(const int* run_start, const int* obj_run_off, const int* obj_hw, const int* obj_out,
                              const int64_t* obj_out_off, uint8_t* out, int64_t out_bytes, int n, seam_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Masks to COCO run-length encoding, csrc/seam_rle.hip: maskApi.c's rleEncode, the opposite direction of the block above.
 * The mask is flattened COLUMN-MAJOR (position p = x*h + y); runs of 0 and 1 alternate, the first a run of zeros.  What the
 * device produces, per object, is the ascending list of positions p with v(p) != v(p-1), v(-1) = 0 (the pixel before (0, x)
 * is (h-1, x-1): a run goes on from the bottom of one column into the top of the next); counts = diff([0, positions, h*w]).
 * A pixel is set iff its byte is non-zero, this project's rule everywhere -- pycocotools' rleEncode compares each byte with
 * its predecessor instead, so it agrees for bytes 0/1 only.
 *
 * An object's workspace is seam_rle_encode_ws_bytes(h, w) = 4 * w * ceil(h/32) bytes (0 for a refused size): one 32-bit word
 * per "cell" of 32 rows x 1 column.  A call works on `cells` = the sum over its objects, object o's first cell at
 * obj_cell_off[o] (the running sum, in cells); ws and counts both hold ws_bytes = 4 * cells bytes and both are cleared by the
 * encode call.  Two steps with the caller's prefix sum between them:
 *   seam_rle_encode_*   ws <- packed value bits, every pixel read (or, for detections, evaluated) exactly once;
 *                       counts int32 [cells] <- transitions per cell, an object's cells in column-major order (column, band).
 *   scan int64 [cells]  the INCLUSIVE prefix sum of counts over the whole table (the caller's: a torch cumsum will do).
 *                       scan[obj_cell_off[o+1] - 1] is the end of object o's positions: the CSR of the result.
 *   seam_rle_positions_* positions int32 [capacity] <- every transition's p at its scanned slot, each slot written once at a
 *                       computed offset.  capacity >= scan[cells-1]; a slot past it is not written.  capacity == 0: no-op.
 * No atomics, no float arithmetic but paste_value's: two calls give identical bytes.  Nothing is allocated, nothing synchronises.
 *
 * _masks: n dense objects, object o the row-major uint8 [h,w] at masks + obj_off[o] (int64 byte offsets, any alignment, the
 *   layout seam_poly_masks_u8 / seam_rle_masks_u8 write; masks holds mask_bytes bytes, an object reaching past them is
 *   skipped).  obj_hw int32 [n][2], obj_off, obj_cell_off are DEVICE tables; obj_hw_host is the same [n][2] table in HOST
 *   memory, read by the launcher to check the shapes and to size the grid.
 * _paste: the D detections of one H x W image, probs [D,28,28], boxes [D,4] xyxy (16-byte aligned): the mask of detection d is
 *   {seam_paste_masks_f32's value > 0.5f}, bit for bit (one device function, csrc/seam_paste.h), the set seam_mask_inter_f32
 *   counts.  Only the clipped integer box is visited; a box that misses the image has no transition.  Object d's cells start
 *   at d * ws_bytes(H, W) / 4.
 * Refused with a non-zero return, nothing launched or written: a NULL pointer (positions may be NULL when capacity == 0), a
 * negative count or size, ws_bytes % 4 or smaller than the objects need, h or w outside 1..16384, h*w >= 2^31.
 * n == 0 / D == 0: no-op, returns 0. */
int64_t seam_rle_encode_ws_bytes(int h, int w);
int seam_rle_encode_masks_u8(const uint8_t* masks, int64_t mask_bytes, const int* obj_hw_host, const int* obj_hw,
                             const int64_t* obj_off, const int64_t* obj_cell_off, void* ws, int64_t ws_bytes, int* counts, int n,
                             seam_stream_t stream);
int seam_rle_encode_paste_f32(const float* probs, const float* boxes, int D, int H, int W, void* ws, int64_t ws_bytes,
                              int* counts, seam_stream_t stream);
int seam_rle_positions_masks(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws,
                             int64_t ws_bytes, const int64_t* scan, int* positions, int64_t capacity, int n, seam_stream_t stream);
int seam_rle_positions_paste(int D, int H, int W, const void* ws, int64_t ws_bytes, const int64_t* scan, int* positions,
                             int64_t capacity, seam_stream_t stream);

/* ---- The bitmap as the common form of the RLE operations (rleMerge, rleIou, rleArea at one bit per pixel) ------------------
 * The workspace layout above ([ceil(h/32)][w] words per object, object o at word obj_cell_off[o]) filled from run lists, combined
 * word by word, counted pair-wise; seam_rle_count_bits + the caller's scan + seam_rle_positions_masks turn any such bitmap back
 * into an RLE.  obj_hw int32 [n][2], obj_cell_off int64 [n] are DEVICE tables (any mix of sizes, the cells of one call's objects
 * need not be adjacent); obj_hw_host is obj_hw in HOST memory, read by the launcher.  Bits of rows at or past h are zero in
 * everything these calls write and are ignored in what they read.  Integer arithmetic only, no atomics: two calls give identical
 * bytes.  Nothing is allocated, nothing synchronises.
 *
 * seam_rle_bits_from_runs: run_start / obj_run_off exactly as seam_rle_masks_u8 takes them, n_runs = obj_run_off[n] entries in
 *   run_start.  One thread per word: a binary search for the run holding the word's first position c*h + 32*band, then a walk
 *   over the runs that start inside its rows.  Every word of every object is written; no other word of ws is.
 * seam_rle_bits_combine: destination object g <- the OR (intersect != 0: the AND) of the source objects group_obj[group_off[g]
 *   .. group_off[g+1]) (int32 DEVICE tables, CSR over n_entries entries, indices into the n_src source objects of src_hw /
 *   src_cell_off / src).  A group's sources have its destination's shape; a source that has not, or an index outside 0..n_src-1,
 *   is left out; a group with no source left gives zeros; a group of one is a copy.  dst and src must not overlap.
 * seam_rle_count_bits: the count stage of seam_rle_encode_* for a bitmap that did not come from there: counts int32, laid out as
 *   ws, <- transitions per cell; only the objects' cells are written (size counts as the objects' cells exactly before a scan).
 * seam_rle_bits_inter: pairs int32 [P][2] (DEVICE), object indices (a, b) of one shape: inter[p] int64 <- sum over the cells of
 *   popcount(a & b), one block per pair, the partial sums joined in a fixed tree.  One launch serves the pairs of many images.
 *   A pair that names an index outside 0..n-1 or two shapes gives -1.
 * seam_rle_bits_area: area[o] int64 <- object o's own popcount (the pair (o, o)).
 * Refused with a non-zero return, nothing launched or written: a NULL table (source tables may be NULL when n_entries == 0), a
 * negative count, h or w outside 1..16384, h*w >= 2^31, ws_bytes % 4 or smaller than the objects need.  n == 0 (n_dst == 0,
 * P == 0): no-op, returns 0. */
int seam_rle_bits_from_runs(const int* run_start, const int* obj_run_off, int n_runs, const int* obj_hw_host, const int* obj_hw,
                            const int64_t* obj_cell_off, void* ws, int64_t ws_bytes, int n, seam_stream_t stream);
int seam_rle_bits_combine(const int* group_off, const int* group_obj, int n_entries, const int* src_hw, const int64_t* src_cell_off,
                          const void* src, int64_t src_bytes, int n_src, const int* dst_hw_host, const int* dst_hw,
                          const int64_t* dst_cell_off, void* dst, int64_t dst_bytes, int n_dst, int intersect, seam_stream_t stream);
int seam_rle_count_bits(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws, int64_t ws_bytes,
                        int* counts, int n, seam_stream_t stream);
int seam_rle_bits_inter(const int* pairs, int P, const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off,
                        const void* ws, int64_t ws_bytes, int n, int64_t* inter, seam_stream_t stream);
int seam_rle_bits_area(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws, int64_t ws_bytes,
                       int n, int64_t* area, seam_stream_t stream);

/* ---- The optimizer step (ref stuffs/engine.py:62-64 optimizer.step(); train_matchrcnn.py:70-72 torch.optim.SGD) ----------------
 * seam_sgd_step_f32: momentum SGD over every tensor of the table in one launch.  `tensors` and `chunks` are DEVICE tables,
 * `groups` is HOST memory and travels by value in the kernel arguments (a changed lr costs no upload).
 *   tensors[t]: p, g (and buf, or NULL without momentum) point at numel fp32 elements, 4-byte aligned; slot indexes groups->g.
 *   chunks[c]:  count <= seam_sgd_chunk_elems() elements of tensor `tensor` from element `offset` (a multiple of that size); the
 *               caller lists every element of every tensor in exactly one chunk and no chunk for an empty tensor.
 *   groups->g[s], per element, every multiply and every add rounded on its own (torch.optim.SGD's arithmetic):
 *       g = maximize ? -grad : grad;  if (weight_decay != 0) g = g + weight_decay * p;
 *       if (momentum != 0) { buf = first ? g : momentum * buf + one_minus_dampening * g;  g = nesterov ? g + momentum * buf : buf; }
 *       p = p - lr * g;
 *     one_minus_dampening is the caller's (1 - dampening) rounded to fp32 once, as torch passes it; `first`: the slot's buffers
 *     are not read, only written.
 * fingerprint: NULL, or 2 * SEAM_SGD_FP_SLOTS uint64 on the device, cleared by the call and filled with partial sums: over the
 *   even entries, the sum modulo 2^64 of (bit pattern x a position-dependent odd weight) of every parameter element as the kernel
 *   READ it; over the odd entries, the same of every element as WRITTEN.  The weights depend on (table index, element index)
 *   only, so with an unchanged parameter list this step's "read" sum equals the previous step's "written" sum unless something
 *   else wrote a parameter in between -- the one kind of edit no version counter shows (`p.data` in torch).  No extra traffic.
 * No byte outside the tensors is written.  Refused (non-zero, nothing launched): n_chunks < 0, groups NULL, groups->n outside
 * 0..SEAM_SGD_MAX_SLOTS, a NULL table with n_chunks > 0.  n_chunks == 0: no-op. */
#define SEAM_SGD_MAX_SLOTS 32
#define SEAM_SGD_FP_SLOTS 64
typedef struct { float* p; const float* g; float* buf; int64_t numel; int group; int slot; } seam_sgd_tensor_t;   /* slot: the clipped step's pending_first index; 0 elsewhere */
typedef struct { int tensor; int count; int64_t offset; } seam_sgd_chunk_t;
typedef struct { float lr, momentum, one_minus_dampening, weight_decay; int nesterov, maximize, first, reserved; } seam_sgd_group_t;
typedef struct { int n; int reserved[3]; seam_sgd_group_t g[SEAM_SGD_MAX_SLOTS]; } seam_sgd_groups_t;
int seam_sgd_chunk_elems(void);
int seam_sgd_step_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                      const seam_sgd_groups_t* groups, unsigned long long* fingerprint, seam_stream_t stream);

/* ---- Gradient clipping by global norm and non-finite steps (torch.nn.utils.clip_grad_norm_; ref stuffs/engine.py:176-181) --------
 * All entries walk the tensor and chunk tables of seam_sgd_step_f32 and use no float atomics.
 * seam_clip_record_t (DEVICE, 8-byte aligned): what the norm leaves for the launches behind it.
 *   total_norm  the global norm over every element of every tensor's g, rounded to fp32 once
 *   clip_coef   clip ? min(1, reciprocal(total_norm + 1e-6f) * max_norm) : 1 -- torch's max_norm / (total_norm + 1e-6) is
 *               Tensor.__rtruediv__, a reciprocal and a multiply, each rounded to fp32; the clamp keeps NaN (total NaN -> NaN,
 *               total inf -> 0)
 *   finite      0 when total_norm is inf or NaN
 *   nonfinite_steps   keep_count ? previous value + !finite : !finite
 * seam_grad_norm_f32: two launches.  Stage 1 (the grid of seam_sgd_step_f32): one fp64 partial per chunk in `workspace`
 *   (seam_grad_norm_workspace_bytes(n_chunks) bytes, 8-byte aligned): norm_inf == 0 the sum of the exact fp64 squares, lane sums in
 *   index order and a fixed tree over lanes and waves; norm_inf != 0 max |g|, NaN if any element is NaN (an explicit flag).  Stage 2
 *   (one block): the partials in chunk order per lane, the same fixed tree, sqrt in fp64 (norm 2), the record.  Two calls on the
 *   same data at the same addresses give the same bits.  Reads nothing outside [g, g + numel); p and buf are not touched.
 *   n_chunks == 0: total_norm 0.
 * seam_grad_scale_f32: g *= record->clip_coef in place (one rounded multiply per element), nothing else written.
 * seam_sgd_step_clip_f32: seam_sgd_step_f32 on g' = g * record->clip_coef (one rounded multiply, what g.mul_(clip_coef) stores; g
 *   itself is only read).  skip_nonfinite != 0 and record->finite == 0: neither p nor buf is written and both fingerprint sums are
 *   the "as read" one.  pending_in / pending_out: two distinct DEVICE int arrays indexed by tensors[t].slot (the caller keeps every
 *   slot inside them).  A tensor is "first" (buf written, not read) when its group slot's `first` is set or pending_in[slot] != 0;
 *   pending_out[slot] = 1 when the launch skipped and the tensor has a buffer and is first, else 0 -- the same value from every
 *   chunk of the tensor.  The caller swaps the two arrays after each call, so a buffer created on a skipped step is written
 *   (buf = g') by the first applied step, whatever dampening and nesterov say.
 * Refused: what seam_sgd_step_f32 refuses; a NULL record / workspace / pending array, pending_in == pending_out, a workspace that
 *   is too small or either pointer not 8-byte aligned. */
typedef struct { float total_norm; float clip_coef; int finite; int reserved; unsigned long long nonfinite_steps; } seam_clip_record_t;
int64_t seam_grad_norm_workspace_bytes(int n_chunks);
int seam_grad_norm_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks, int norm_inf, int clip,
                       float max_norm, int keep_count, void* workspace, int64_t workspace_bytes, seam_clip_record_t* record,
                       seam_stream_t stream);
int seam_grad_scale_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                        const seam_clip_record_t* record, seam_stream_t stream);
int seam_sgd_step_clip_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                           const seam_sgd_groups_t* groups, unsigned long long* fingerprint, const seam_clip_record_t* record,
                           int skip_nonfinite, const int* pending_in, int* pending_out, seam_stream_t stream);

/* seam_repack_many_f32: the fp32 weight packs of a list of (layer, form) jobs in one launch, each job's bytes equal to its
 * per-layer entry's: IGEMM = seam_pack_conv_weight_f32 (modes 0, 1, 2), SPLIT3 = seam_pack_conv_weight_sx (computed from the
 * source, no scratch), WINO / WINO24 = seam_pack_conv_weight_wino_f32 / _wino24_f32, PC = seam_pack_conv1x1_pc_f32, NARROW =
 * seam_pack_linear_narrow_f32, SXPC = seam_pack_conv1x1_weight_sxpc, SW = the row-major [K, C] weights of seam_conv1x1_sw_f32 with scale[k] folded into row k
 * (scale NULL: a copy).  1x1 forms (PC, SXPC, SW, NARROW) take R = S = 1, Cstore = Cin = C, mode 0.
 * seam_repack_layout (HOST table) checks every job by its per-layer entry's rules and fills kred, rows, items, first_block and
 * n_blocks; it returns the launch's block count, or -(1 + k) when job k is refused.  The caller copies the table to the device
 * and passes that copy, the job count and the block count to seam_repack_many_f32. */
enum { SEAM_REPACK_IGEMM = 0, SEAM_REPACK_WINO = 1, SEAM_REPACK_WINO24 = 2, SEAM_REPACK_PC = 3, SEAM_REPACK_SW = 4,
       SEAM_REPACK_SPLIT3 = 5, SEAM_REPACK_NARROW = 6, SEAM_REPACK_SXPC = 7,
       SEAM_REPACK_SXPC64 = 8 /* the same item function for the shapes of seam_conv1x1_sxpc64_supported (K == 64) and of
                                 seam_conv1x1_sxpc_short_supported (C == 128) */,
       SEAM_REPACK_W24SX = 9 /* seam_pack_conv_weight_wino24_sx (R = S = 3, modes 0 and 2) */ };
typedef struct {
    const float* src; void* dst; const float* scale;
    int64_t items;
    int form, K, Cin, R, S, Cstore, mode;
    int kred, rows, first_block, n_blocks, reserved;
} seam_repack_job_t;
long long seam_repack_layout(seam_repack_job_t* jobs, int n_jobs);
int seam_repack_many_f32(const seam_repack_job_t* jobs, int n_jobs, long long total_blocks, seam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEAM_HIP_H */
