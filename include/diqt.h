/*
 * diqt.h — C ABI of libdiqt_hip.so: the MI355X (gfx950) device kernels behind the
 * DiffusionIQT hot path (3-D conditional-diffusion U-Net forward/backward, DDPM/EDM sampler
 * step, loss, optimiser step).
 *
 * Drop-in boundary: the reference has no native layer — every FLOP is an ATen op
 * called from imagen_pytorch3D.py / imagen_video.py / elucidated_imagen.py / trainer.py.  Each entry
 * point below names the reference call site(s) (file:line, relative to the reference root) whose
 * ATen op(s) it replaces.  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only: device pointers, ints, floats; `stream` is a hipStream_t passed as void*
 *     (NULL = the null stream).  Every call is asynchronous on `stream`, holds no pointer past the
 *     completion of the work it enqueues and keeps no global mutable state.
 *   - activations are fp32, channels-last ("NDHWC"): x[b][d][h][w][c], c fastest.
 *     `rows` = b*d*h*w when an op does not care about the spatial structure.
 *   - weights cross the boundary in the reference's own layout (OIDHW for Conv3d, [out][in] for
 *     Linear); diqt_conv_pack_weight re-lays them for the MFMA kernels.
 *   - every entry returns DIQT_OK (0) or a negative DIQT_E_* code; it never throws, never exits.
 *     diqt_last_error() returns a thread-local message for the most recent failure.
 */
#ifndef DIQT_H
#define DIQT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIQT_OK             0
#define DIQT_E_SHAPE       -1   /* an extent is <= 0 or inconsistent with another          */
#define DIQT_E_ALIGN       -2   /* a pointer is NULL or not aligned as the kernel requires  */
#define DIQT_E_UNSUPPORTED -3   /* valid request the library has no kernel for              */
#define DIQT_E_LAUNCH      -4   /* HIP reported an error at launch                          */
#define DIQT_E_WORKSPACE   -5   /* workspace too small (see the *_workspace_bytes query)    */

/* activation selectors (imagen_pytorch3D.py:547 Mish; imagen_video.py:690 SiLU; :1113 GELU; :623 ReLU; :625 Sigmoid) */
#define DIQT_ACT_NONE    0
#define DIQT_ACT_MISH    1
#define DIQT_ACT_SILU    2
#define DIQT_ACT_GELU    3
#define DIQT_ACT_RELU    4
#define DIQT_ACT_SIGMOID 5

int         diqt_version(void);
const char* diqt_last_error(void);

/* Launch census (test / measurement infrastructure, no reference counterpart: the reference dispatches through ATen and can be
 * watched with torch.profiler).  Every kernel launch of the library carries a tag (the names diqt_last_error reports, e.g.
 * "conv3d_fwd_h(persistent)", "conv3d_fwd(v9)", "temporal_attention_h").  diqt_census_enable(1) zeroes the per-tag counters and
 * starts counting, (0) stops; both return the previous state.  diqt_census_count(s) = launches since then whose tag contains s
 * (NULL: all).  diqt_get_last_launch() = tag of the calling thread's most recent launch.  Thread-safe. */
int         diqt_census_enable(int on);
long long   diqt_census_count(const char* substr);
const char* diqt_get_last_launch(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution (stride 1, zero padding) as an im2col-free implicit GEMM on v_mfma_f32_32x32x2_f32.
 * Replaces nn.Conv3d / nn.Linear / nn.Conv1d at: Block.project imagen_pytorch3D.py:551-553,566;
 * init_conv :1289-1291,1589; 1x1 convs :467,495,597,1388,1477; Linear :588,622-624,1310,1315;
 * pseudo-3D convs imagen_video.py:352-406,529-543.
 * Output extent per axis: O = I + 2*pad + epad - k + 1, where pad is the low-side (and, with epad = 0, the
 * high-side) zero padding and `epad` is EXTRA high-side padding (may be negative): the causal temporal
 * convolutions of imagen_video.py:399-402 / :1351-1352 are pad = k-1, epad = -(k-1).
 * ---------------------------------------------------------------------------------------------- */

/* number of floats in the packed-weight buffer for a (Cout,Cin,kd,kh,kw) filter */
size_t diqt_conv_packed_elems(int Cout, int Cin, int kd, int kh, int kw);

/* floats of the Winograd F(2,3) panels that pack modes 2 / 3 append behind the direct pack, for an effective
 * (out, in) = (Cout, Cin) filter: nonzero for 3x3x3 filters with in % 16 == 0                        */
size_t diqt_conv_packed_wino_elems(int Cout, int Cin, int kd, int kh, int kw);

/* mode 0: forward packing of w[Cout][Cin][kd][kh][kw];
 * mode 1: backward-data packing (taps flipped, in/out swapped) — feed to diqt_conv3d_fwd with
 *         (Cin,Cout) swapped and pad' = k-1-pad to obtain dX from dY.
 * mode 2 / 3: the packing of mode 0 / 1 followed by the Winograd panels of the same effective filter
 *         (diqt_conv_packed_elems + diqt_conv_packed_wino_elems floats).  Only the *_pk entry points,
 *         told the buffer's length, read the panels; every other entry point reads the direct pack. */
int diqt_conv_pack_weight(const float* w_oidhw, float* packed, int Cout, int Cin,
                          int kd, int kh, int kw, int mode, void* stream);

/* y[B][Do][Ho][Wo][Cout] = conv(x[B][D][H][W][Cin], packed) + bias   (bias may be NULL).
 * If `residual` != NULL it is added in the epilogue (same shape as y).                              */
int diqt_conv3d_fwd(const float* x, const float* packed, const float* bias, const float* residual,
                    float* y, int B, int D, int H, int W, int Cin, int Cout,
                    int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);

/* Mixed-precision forward conv (v_mfma_f32_32x32x16_f16 / _bf16, fp32 accumulate): the autocast path of the samplers.
 * Replaces ATen's autocast policy for conv3d / linear -- `torch.autocast` around `ElucidatedImagen.sample` and
 * `ImagenTrainer(fp16=True)` -> `Accelerator(mixed_precision='fp16')` (trainer.py:293-311): operands are cast to fp16 (bf16 = 1:
 * bf16) while the halo tile is staged, products accumulate in fp32, and with round_out = 1 the result (+ bias) is rounded once to
 * the operand type before the fp32 store, as an fp16 output tensor would be.  x, y, bias, residual stay fp32 NDHWC.
 * `packed_h`: 16-bit [ci/32][tap][co padded to 64][32] from diqt_conv_pack_weight_h (diqt_conv_packed_h_elems elements of the
 * EFFECTIVE out/in channel counts).  With the mode-1 packing the same entry point computes backward-data (dX from dY), which the
 * bf16 training path uses; fp16 gradients would need loss scaling and stay on the fp32 kernel.
 * diqt_conv3d_fwd_h_supported() == 0 (Cin % 4 != 0, a tensor >= 1 GiB, halo tile beyond the LDS): stay on diqt_conv3d_fwd.   */
size_t diqt_conv_packed_h_elems(int Cout, int Cin, int kd, int kh, int kw);
int diqt_conv_pack_weight_h(const float* w_oidhw, void* packed_h, int Cout, int Cin, int kd, int kh, int kw, int mode, int bf16,
                            void* stream);
/* `count` such packs in one launch per 64 rows: host_table rows of 8 x int64 {w (device pointer), packed_h (device pointer), Cout, Cin, kd,
 * kh, kw, mode} travel in the kernel arguments (what the captured training micro-step replays to re-derive every packed copy). */
int diqt_conv_pack_weight_h_multi(const long long* host_table, int count, int bf16, void* stream);   /* mode as in diqt_conv_pack_weight: 1 = flipped / swapped packing for backward-data */
int diqt_conv3d_fwd_h_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                int epd, int eph, int epw);
/* diqt_conv3d_fwd_h with 16-bit tensors at either end: x_half: x holds values of the operand type (fp16, or bf16 when `bf16`) instead of
 * fp32; y_half: y is stored in that type (needs round_out and no residual).  The two convs of a pseudo-3D block (per-frame k x k, then
 * temporal; imagen_video.py:352-406) pass their intermediate tensor this way: the same values the fp32 tensor would hold -- autocast
 * rounds a conv's result to the operand type -- at half the bytes.  Only where ..._io16_supported says 1 (the persistent kernel's
 * shapes, Cin and Cout multiples of 8).                                                                                        */
int diqt_conv3d_fwd_h_io16_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                     int epd, int eph, int epw, int x_half, int y_half);
/* stats (may be NULL): per-(tile, wave) column sums (sum, sum of squares) of the stored values for the consumer's GroupNorm,
 * [B][nblk][2][Cout] with nblk = diqt_conv3d_fwd_h_stats_blocks(...) (0: none for this shape); feed them to
 * diqt_groupnorm_stats_from_partials -- the statistics pass over the tensor disappears.                                        */
int diqt_conv3d_fwd_h_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                   int epd, int eph, int epw, int x_half, int y_half);
int diqt_conv3d_fwd_h_io(const void* x, const void* packed_h, const float* bias, const float* residual, void* y, int B, int D, int H,
                         int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, int bf16,
                         int round_out, int x_half, int y_half, float* stats, void* stream);
/* diqt_conv3d_fwd_h walks (tile, channel-block) units with a persistent kernel of this many workgroups (default 256, one per CU)
 * when a launch has at least twice as many units and the halo tile fits the register prefetch; n > 0 sets the count, n <= 0 only
 * queries; returns the previous value.  Results do not depend on it.                                                            */
int diqt_set_convh_workgroups(int n);
/* diqt_conv3d_fwd_h_io with x_half = 1 on a 3x3x3 or (1,3,3) filter (Cin % 32 == 0, Cout % 8 == 0) runs conv_f9h_kernel -- halo images by
 * LDS-DMA, one wave per SIMD, weight fragments streamed into registers -- when mode = 1 (default) and the tiles fill the
 * chip, for any tile count when mode = 2, never when 0.  mode >= 0 sets it, mode < 0 only queries; returns the previous value.  Results
 * agree with the other 16-bit kernels bit for bit on integer-valued data (different K order otherwise).                          */
int diqt_set_conv_f9h_mode(int mode);
/* Diagnostic, the counterpart of diqt_conv3d_fwd_kernel_id: the kernel a diqt_conv3d_fwd_h / diqt_conv3d_fwd_h_io call with round_out = 1
 * runs for this shape, these tensor types and the current run-time switches (the launch takes its decision from the same function) --
 * 0 unsupported (the call returns an error and launches nothing), 1 conv_fwd_h_kernel with halo prefetch, 2 conv_fwd_h_kernel without,
 * 3 conv_fwd_hp_kernel on 8 waves, 4 the same staging two 32-channel chunks of a pointwise conv per step, 5 conv_fwd_hp_kernel on 4 waves,
 * 6 conv_pw_h_kernel on a pointwise conv, 7 conv_pw_h_kernel on a temporal conv, 8 conv_f9h_kernel.                                      */
int diqt_conv3d_fwd_h_kernel_id(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                int epd, int eph, int epw, int x_half, int y_half, int has_residual, int has_stats);
/* the conv_f9h_kernel variant (0..5; 6-8: the split builds of diqt_conv3d_fwd_split16*, 9: its tap-paired build) the process's last launch of it ran, -1 if none since the previous call (read and clear) */
int diqt_get_last_conv_f9h_variant(void);
int diqt_conv3d_fwd_h(const float* x, const void* packed_h, const float* bias, const float* residual, float* y, int B, int D, int H,
                      int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, int bf16,
                      int round_out, void* stream);

/* fp32 3x3x3 forward conv on the fp16 matrix pipe by the three-product split (conv_split16.hip): each operand is an fp16 head plus an fp16
 * tail scaled by 2^11, x w ~= xh wh + 2^-11 (xh wl + xl wh), summed in fp32 -- fp32-sized error (below the Winograd tile's), three
 * 16-bit MFMAs for sixteen f32 ones.  Domain: |w| < 65504 (the pack sets *refused = 1 otherwise: keep the layer on diqt_conv3d_fwd*);
 * an activation beyond +-65504 is clamped (finite output, accuracy lost).  x, y, bias, residual, stats: fp32 as for diqt_conv3d_fwd_pk.
 * x16: scratch of B D H W Cin * 4 bytes for the split activations (NDHWC, per 16 channels [16 heads | 16 tails]).  packed: 16-bit
 * [ci/16][tap][co padded to 64][16 heads | 16 tails], diqt_conv_packed_split16_elems elements.  ..._supported: Cin % 16 == 0,
 * Cout % 8 == 0, what conv_f9h_kernel's planner takes at 2 Cin channels, and at least 128 (tile, 64-channel block) units unless
 * diqt_set_conv_f9h_mode(2).  stats (may be NULL): [B][diqt_conv3d_fwd_split16_stats_blocks][2][Cout] column sums of y.
 * The _gn form applies act(A x + Bc), coef = [2][B][Cin] as for diqt_conv3d_fwd_gn, in the pass that splits x.                  */
size_t diqt_conv_packed_split16_elems(int Cout, int Cin, int kd, int kh, int kw);
int diqt_conv_pack_weight_split16(const float* w_oidhw, void* packed, int* refused, int Cout, int Cin, int kd, int kh, int kw, void* stream);
int diqt_conv3d_fwd_split16_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                      int epd, int eph, int epw);
int diqt_conv3d_fwd_gn_split16_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                         int epd, int eph, int epw, int act);
int diqt_conv3d_fwd_split16_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                         int epd, int eph, int epw);
int diqt_conv3d_fwd_split16_variant(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                    int epd, int eph, int epw);
int diqt_conv3d_fwd_split16(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y, float* stats,
                            int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph,
                            int epw, void* stream);
int diqt_conv3d_fwd_gn_split16(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                               float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                               int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
/* The fill plan of the same route (conv_split16_b.hip), for launches whose 256-voxel tiles leave CUs without a workgroup: the 256-,
 * 128- and 64-voxel tiles (variants 6, 7, 8) are tried in that order, a smaller one only when the larger gives fewer than 256 (tile,
 * 64-channel block) units; granted at 128 units or more and B Do Ho Wo Cin Cout >= 2^25 (diqt_set_conv_f9h_mode(2) lifts both floors).
 * y is bit-identical to the plan above on a shape both take; the statistics have ..._fill_stats_blocks rows.  The arguments of the
 * namesakes above.  diqt_set_conv_split16_fill_tile(6 | 7 | 8) pins the tile under mode 2 (tests), 0 unpins, < 0 queries; returns the
 * previous value.                                                                                                                  */
int diqt_set_conv_split16_fill_tile(int variant);
int diqt_conv3d_fwd_split16_fill_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                           int epd, int eph, int epw);
int diqt_conv3d_fwd_gn_split16_fill_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                              int epd, int eph, int epw, int act);
int diqt_conv3d_fwd_split16_fill_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                              int epd, int eph, int epw);
int diqt_conv3d_fwd_split16_fill_variant(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                         int epd, int eph, int epw);
int diqt_conv3d_fwd_split16_fill(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                 float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                 int epd, int eph, int epw, void* stream);
int diqt_conv3d_fwd_gn_split16_fill(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                    float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                                    int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
/* The pair plan of the same route (conv_split16_c.hip): the 256-voxel tile on a tap-paired v_mfma_f32_16x16x32_f16 body (variant 9; two
 * taps per product, two accumulator sets), the same x16, packed weights, tiling and statistics rows as variant 6.  Granted for 3x3x3
 * filters with Cin % 16 == 0 at 256 (tile, 64-channel block) units or more, B Do Ho Wo Cin Cout >= 2^25 and, where every workgroup has a
 * single tile (units <= workgroups), Cin >= 128 = eight chunks of 16 channels (diqt_set_conv_f9h_mode(2) lifts the three floors).  y differs from variant 6's in the last bits (another order of the fp32 sums).  The arguments of the namesakes
 * above.  diqt_conv_split16_pair_lds_conflicts (host only): the worst number of distinct addresses on one 16-byte LDS slot among the
 * lanes a ds_read_b128 serves together, over all fragment reads of the body; 1 = conflict-free.                                      */
int diqt_conv3d_fwd_split16_pair_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                           int epd, int eph, int epw);
int diqt_conv3d_fwd_gn_split16_pair_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                              int epd, int eph, int epw, int act);
int diqt_conv3d_fwd_split16_pair_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                              int epd, int eph, int epw);
int diqt_conv3d_fwd_split16_pair(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                 float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                 int epd, int eph, int epw, void* stream);
int diqt_conv3d_fwd_gn_split16_pair(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                    float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                                    int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
int diqt_conv_split16_pair_lds_conflicts(void);

/* Forward conv that also emits per-tile column sums of its OUTPUT for the consumer's GroupNorm statistics / SE pooling
 * (Block -> Block and Block -> SE3D inside ResnetBlock, imagen_pytorch3D.py:568-632): stats[B][nblk][2][Cout] =
 * (sum, sum of squares) over the valid voxels of each output tile, nblk = diqt_conv3d_fwd_stats_blocks(...) (0: this shape
 * takes a path without statistics and `stats` must be NULL).  Saves one full read of the tensor per consumer.            */
/* Diagnostic: the kernel diqt_conv3d_fwd* runs for this shape -- 0 conv_fwd_kernel, 1 conv_fwd_smallcin_kernel, 2 conv1x1_fwd_kernel,
 * 3 conv_fwd8_kernel, 4 conv_fwd9_kernel (incl. its split-K form, taken when the caller passes the workspace that
 * diqt_conv3d_fwd_workspace_bytes asks for) (-1: bad shape) -- so that per-kernel timings taken around the call carry the names
 * rocprofv3 reports.                                                                                                               */
int diqt_conv3d_fwd_kernel_id(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                              int epd, int eph, int epw);
/* conv_fwd9_kernel's variant for a launch that diqt_conv3d_fwd_kernel_id routes to it, given a packed buffer of
 * packed_elems floats (7: the Winograd F(2,3) 3x3x3 tile of diqt_conv3d_fwd_pk), else -1 */
int diqt_conv3d_fwd9_variant(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                             int epd, int eph, int epw, size_t packed_elems);
/* Diagnostic: the decision every fp32 forward launch and every query above reads (one function in conv_mfma.hip), as a pure shape
 * query for one ask: a diqt_conv3d_fwd_pk call (sub_f = 0, gn_act = 0), a diqt_conv3d_fwd_neighbours call (sub_f = f) or a
 * diqt_conv3d_fwd_gn_pk call (gn_act = its activation) with a packed buffer of packed_elems floats, with / without a workspace and
 * a statistics buffer.  `field` 0 the kernel, numbered as diqt_conv3d_fwd_kernel_id (-1: the call is refused), 1 the split-K shares,
 * 2 conv_fwd9_kernel's variant or -1, 3 the statistics rows granted to this ask (0: the launch is the one without statistics and
 * `stats` must be NULL; a GroupNorm-apply launch that splits K is granted none), 4 the workspace bytes the launch uses (saturating
 * at INT_MAX); another field: -1.                                                                                                  */
int diqt_conv3d_fwd_route(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                          int epd, int eph, int epw, size_t packed_elems, int has_workspace, int has_stats, int sub_f, int gn_act,
                          int field);
/* the conv_fwd9_kernel variant the process's last launch of it ran, -1 if none since the previous call (read and clear) */
int diqt_get_last_conv_fwd9_variant(void);
int diqt_conv3d_fwd_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                 int epd, int eph, int epw);
int diqt_conv3d_fwd_ex(const float* x, const float* packed, const float* bias, const float* residual, float* y, float* stats,
                       void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int Cin, int Cout,
                       int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
/* diqt_conv3d_fwd_ex told the length of the packed buffer (floats).  A buffer from pack mode 2 (direct pack + Winograd panels)
 * lets 3x3x3 launches with an even output width run conv_fwd9_kernel's Winograd F(2,3) tile (4 MFMA products per output pair
 * instead of 6; DIQT_CONV_F9W=0 in the environment keeps the direct tiles); a buffer of diqt_conv_packed_elems floats gives the
 * direct tiles exactly as diqt_conv3d_fwd_ex; a shorter one is refused (DIQT_E_SHAPE).  The Winograd tile has its own tile count,
 * so statistics rows and split-K workspace come from the _pk queries with the same length.                                     */
int diqt_conv3d_fwd_pk(const float* x, const float* packed, size_t packed_elems, const float* bias, const float* residual, float* y,
                       float* stats, void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int Cin, int Cout,
                       int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
/* 1x1x1 conv with an extended epilogue (fp32, no workspace, never split): act 0 / DIQT_ACT_MISH on acc + bias; d2s: depth-to-space by 2
 * of the result, y[B][2D][2H][2W][Cout / 8], with `packed` / `bias` from diqt_conv1x1_pack_d2s (Cout / 8 a multiple of 64); stats: rows
 * of column sums [B][nblk][2][C] of the final output, nblk = diqt_conv1x1_fwd_ex_stats_blocks (0: D H W is no multiple of 128); h and
 * gate (together): y = gate[b][co] * h[row][co] + (acc + bias), always with stats.  The forms: Mish + d2s [+ stats], stats, gated;
 * diqt_conv1x1_fwd_ex_supported = 0: use diqt_conv3d_fwd* and the separate passes.  Results equal those passes bit for bit; only the
 * summation order of the statistics is this kernel's own (fixed, no atomics).                                                        */
int diqt_conv1x1_fwd_ex_supported(int B, int D, int H, int W, int Cin, int Cout, int act, int d2s, int stats, int gated);
int diqt_conv1x1_fwd_ex_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int act, int d2s, int gated);
int diqt_conv1x1_pack_d2s(const float* w, const float* bias, float* packed, float* bias_packed, int Cout, int Cin, void* stream);
int diqt_conv1x1_fwd_ex(const float* x, const float* packed, const float* bias, const float* h, const float* gate, float* y, float* stats,
                        int B, int D, int H, int W, int Cin, int Cout, int act, int d2s, void* stream);
int diqt_conv3d_fwd_stats_blocks_pk(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                    int epd, int eph, int epw, size_t packed_elems);
size_t diqt_conv3d_fwd_workspace_bytes_pk(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                                          int pd, int ph, int pw, int epd, int eph, int epw, size_t packed_elems);
/* consumers of such partials */
int diqt_groupnorm_stats_from_partials(const float* partials, float* mean, float* rstd, int B, int nblk, int rows_per_batch,
                                       int C, int G, float eps, void* stream);
int diqt_channel_mean_from_partials(const float* partials, float* pooled, int B, int nblk, int rows_per_batch, int C, void* stream);

/* 'same' convolution (odd cubic filter k, padding k/2) over the f^3 sub-volume batch x[f^3][A][A][A][Cin] of ONE merged (fA)^3
 * volume (entry n = b2 + f b3 + f^2 b4, utils_mine.py:25-67), each sub-volume's halo read IN PLACE from its neighbours and zero
 * only outside the merged volume: the reference's boundary_pad (merge_sub_volumes -> F.pad -> overlapping unfold,
 * imagen_pytorch3D.py:37-46) followed by the unpadded Conv3d of Block.forward (:550-566, boundary=True), without the merged and
 * re-split copies.  Same kernels (conv_fwd8 / conv_fwd / small-Cin) and bits as running those copies through them.  stats:
 * [f^3][diqt_conv3d_fwd_neighbours_stats_blocks][2][Cout]; workspace as diqt_conv3d_fwd_ex for (B = f^3, D = H = W = A, pad = k/2).
 * The batch must stay below 1 GiB. */
int diqt_conv3d_fwd_neighbours_stats_blocks(int f, int A, int Cin, int Cout, int k);   /* rows per batch entry of `stats` (0: none) */
int diqt_conv3d_fwd_neighbours(const float* x, const float* packed, const float* bias, const float* residual, float* y, float* stats,
                               void* workspace, size_t workspace_bytes, int f, int A, int Cin, int Cout, int k, void* stream);

/* Same operator with a caller-owned workspace: launches too small to fill the chip (8^3 / 16^3 levels) slice the
 * input-channel chunks over grid.y into output slabs and a second kernel sums them (+ bias + residual) in a fixed
 * order.  diqt_conv3d_fwd_workspace_bytes() returns 0 when the shape is not split.                              */
size_t diqt_conv3d_fwd_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                                       int pd, int ph, int pw, int epd, int eph, int epw);
int diqt_conv3d_fwd_ws(const float* x, const float* packed, const float* bias, const float* residual,
                       float* y, void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int Cin, int Cout,
                       int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);

/* LDS bytes the MFMA kernel needs for this geometry (> 160 KiB: use diqt_conv3d_direct_*); < 0 on bad shape */
long long diqt_conv3d_lds_bytes(int D, int H, int W, int kd, int kh, int kw, int pd, int ph, int pw,
                                int epd, int eph, int epw);

/* Which kernel diqt_conv3d_bwd_weight dispatches a shape to (profilers / bench.py: per-kernel numbers under rocprofv3's names):
 * 3 conv_wgrad3_kernel (one wave per SIMD, LDS-DMA double-buffered tiles), 2 conv_bwd_weight2_kernel, 1 conv_bwd_weight_kernel,
 * 0 a GEMM / column-sum path (un-padded 1x1x1 filters, <= 4 input channels), -1 bad shape: the route below for aligned pointers. */
int diqt_conv3d_bwd_weight_kernel_id(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                     int epd, int eph, int epw);
/* Diagnostic: the decision diqt_conv3d_bwd_weight itself obeys, for a call whose x, dy and dw are all 16-byte aligned (`aligned`) or not,
 * with (`want_bias`) or without dbias.  field 0: kernel id as above; 1: path, in the order the launch tries them -- 0 weighted column sum
 * (un-padded 1x1x1 filter, Cout == 1), 1 im2col + split-K GEMM (<= 4 input channels), 2 1x1x1 split-K GEMM, 3 conv_wgrad3_kernel,
 * 4 conv_bwd_weight2_kernel, 5 conv_bwd_weight_kernel, -1 the launch refuses; 2: split-K shares; 3: 1 when the bias gradient rides on the
 * kernel (partials behind the slabs) instead of taking the two-stage column sum; 4: workspace bytes this launch uses (at most
 * diqt_conv3d_bwd_weight_workspace_bytes, which every launch asks for; clamped to INT_MAX); 5: the launch's return code for a valid call
 * (DIQT_OK or the refusal's code); another field: -1. */
int diqt_conv3d_bwd_weight_route(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                 int epd, int eph, int epw, int aligned, int want_bias, int field);

/* dW[Cout][Cin][kd][kh][kw] (OIDHW, overwritten) and dbias[Cout] (may be NULL) from x and dY.
 * Deterministic: split-K partial slabs in `workspace` are reduced in a fixed order.                  */
size_t diqt_conv3d_bwd_weight_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout,
                                              int kd, int kh, int kw, int pd, int ph, int pw,
                                              int epd, int eph, int epw);
int diqt_conv3d_bwd_weight(const float* x, const float* dy, float* dw_oidhw, float* dbias,
                           void* workspace, size_t workspace_bytes,
                           int B, int D, int H, int W, int Cin, int Cout,
                           int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);

/* The weight gradient with 16-bit MFMA operands (bf16 when `bf16`, else fp16; fp32 accumulate): x and dY are rounded to that type while
 * staged, as the reference's autocast backward does under `ImagenTrainer(precision='bf16')` (trainer.py:293-311).  dbias is summed from the
 * fp32 dY.  3x3x3, (1,3,3), (3,1,1) filters, Cin % 32 == 0; ..._workspace_bytes == 0: shape not taken -- use diqt_conv3d_bwd_weight.  Deterministic.
 * Bit 2 of `bf16` (value 4): dY holds 16-bit values of the operand type too (the gradient a low-precision training step keeps in that type).
 * Bit 1 of `bf16` (value 2): x already HOLDS 16-bit values of the operand type (the GroupNorm-apply output a bf16 training step kept in
 * that type for the conv's forward and for this pass: half the bytes, the same bits the fp32 values round to).                          */
size_t diqt_conv3d_bwd_weight_h_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                int pw, int epd, int eph, int epw);
/* 1 when diqt_conv3d_bwd_weight_h takes this shape with these flag bits (2: 16-bit x, 4: 16-bit dY -- only together with a 16-bit x, and
 * Cout % 8 == 0), else 0: the call returns an error and launches nothing.  flags = 0 agrees with ..._workspace_bytes > 0.               */
int diqt_conv3d_bwd_weight_h_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                       int epd, int eph, int epw, int flags);
int diqt_conv3d_bwd_weight_h(const float* x, const float* dy, float* dw_oidhw, float* dbias, void* workspace, size_t workspace_bytes,
                             int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd,
                             int eph, int epw, int bf16, void* stream);

/* Stride-1 convolution with one or two output channels (the U-Nets' final convs dim -> channels, imagen_video.py:1560,
 * imagen_pytorch3D.py:1485; GlobalContext.to_k, imagen_video.py:585-601) on the vector ALU: per halo voxel the responses of all taps
 * from ONE pass over x, then a T-point gather.  Exact fp32; OIDHW weights as they are (no packing); any Cin >= 16.
 * Filters 1x1x1, (1,3,3), (3,1,1), 3x3x3 with Cout = 1 and 1x1x1, (1,3,3) with Cout = 2 (..._supported).                    */
int diqt_conv3d_fwd_smallcout_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                        int epd, int eph, int epw);
int diqt_conv3d_fwd_smallcout(const float* x, const float* w_oidhw, const float* bias, const float* residual, float* y, int B, int D,
                              int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw,
                              void* stream);

/* Direct (non-MFMA) grouped / strided convolution for the FLOP-trivial shapes: depthwise 3^3 and
 * patchify k=s=p convs of the attention blocks (imagen_pytorch3D.py:858-869, 913-924, 960-976),
 * temporal depthwise (3,1,1) PEG (imagen_video.py:1351-1352).  Weights OIDHW with I = Cin/groups.   */
int diqt_conv3d_direct_fwd(const float* x, const float* w, const float* bias, float* y,
                           int B, int D, int H, int W, int Cin, int Cout, int groups,
                           int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                           int epd, int eph, int epw, void* stream);
int diqt_conv3d_direct_bwd_data(const float* dy, const float* w, float* dx,
                                int B, int D, int H, int W, int Cin, int Cout, int groups,
                                int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                                int epd, int eph, int epw, void* stream);
int diqt_conv3d_direct_bwd_weight(const float* x, const float* dy, float* dw, float* dbias,
                                  int B, int D, int H, int W, int Cin, int Cout, int groups,
                                  int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                                  int epd, int eph, int epw, void* stream);
/* Same gradients reduced over the voxel slices in a fixed order through `workspace` (no atomics: bit-reproducible). */
size_t diqt_conv3d_direct_bwd_weight_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout, int groups, int kd, int kh,
                                                     int kw, int sd, int sh, int sw, int pd, int ph, int pw, int epd, int eph, int epw);
int diqt_conv3d_direct_bwd_weight_ws(const float* x, const float* dy, float* dw, float* dbias, void* workspace,
                                     size_t workspace_bytes, int B, int D, int H, int W, int Cin, int Cout, int groups,
                                     int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int epd, int eph,
                                     int epw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm + (scale+1)*x+shift + activation  — Block.forward imagen_pytorch3D.py:555-562,
 * imagen_video.py:683-699.  Statistics per (batch, group) over rows_per_batch x (C/G).
 * ---------------------------------------------------------------------------------------------- */
/* workspace: diqt_reduce_workspace_bytes(B, C) bytes, 16-byte aligned (per-(b,c) partial moments) */
size_t diqt_reduce_workspace_bytes(int B, int C);
int diqt_groupnorm_stats(const float* x, float* mean, float* rstd, void* workspace, size_t workspace_bytes,
                         int B, int rows_per_batch, int C, int G, float eps, void* stream);
/* The plan of every column reduction over [rows][C] (GroupNorm statistics and backward, LayerNorm dg / db, channel means), as a pure
 * shape query (no GPU): `field` 0 workgroups per batch element, 1 rows per workgroup (past 64 * 256 rows the last workgroups may start
 * beyond `rows` and write zero partials), 2 whether the channel-quad path runs (C % 4 == 0, C <= 1024), 3 the rows a workgroup reads in
 * parallel on that path (0 otherwise).  -1: bad shape or field.                                                                      */
int diqt_colreduce_route(int rows, int C, int field);
/* The decisions of the GroupNorm apply launches (diqt_gn_act_fwd / _fwd_h, the dx pass of diqt_gn_act_bwd*): `field` 0 whether the
 * vectorised kernel runs (C % 4 == 0, rows * C % 4 == 0 and `all_aligned`: every tensor pointer 16-byte aligned), 1 grid.x.         */
int diqt_gn_apply_route(int B, int rows_per_batch, int C, int all_aligned, int field);

/* y = act( ((x-mean)*rstd*gamma+beta) * (scale+1) + shift ); scale/shift are both NULL or point at
 * rows of `cond_stride` floats per batch element (the reference chunks one [B][2C] time embedding,
 * imagen_pytorch3D.py:603-605: scale = emb, shift = emb + C, cond_stride = 2C).                       */
int diqt_gn_act_fwd(const float* x, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, const float* scale, const float* shift,
                    int cond_stride, float* y, int B, int rows_per_batch, int C, int G, int act, void* stream);
/* The same with y stored in fp16 (bf16 when `bf16`): under autocast the consumer is a 16-bit-operand conv (diqt_conv3d_fwd_h_io,
 * x_half) that would round these values to that type while staging them.  x_half: x is itself the 16-bit output of such a conv
 * (y_half; its GroupNorm statistics come from that conv's `stats`).  Needs C % 4 == 0 and 16-byte aligned tensors.               */
int diqt_gn_act_fwd_h(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* scale,
                      const float* shift, int cond_stride, void* y_h, int B, int rows, int C, int G, int act, int bf16, int x_half,
                      void* stream);

/* dx, dgamma[C], dbeta[C], dscale[B][C], dshift[B][C] (last two NULL when scale/shift are).
 * `workspace` holds per-(b,c) partial sums: diqt_reduce_workspace_bytes(B,C).                         */
int diqt_gn_act_bwd(const float* x, const float* dy, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, const float* scale, const float* shift,
                    int cond_stride, float* dx, float* dgamma, float* dbeta, float* dscale, float* dshift,
                    void* workspace, size_t workspace_bytes,
                    int B, int rows_per_batch, int C, int G, int act, void* stream);

/* The GroupNorm + activation backward split around the conv it feeds (Block = GN -> act -> conv): diqt_conv3d_fwd_gnbwd is the
 * conv's backward-data pass (x = gradient of the conv output, flipped packed weights) whose epilogue also reduces the GroupNorm
 * backward's per-channel sums over each output tile, reading the GroupNorm input gn_x at the tile's voxels:
 * partials[B][nblk][2][Cout], nblk = diqt_conv3d_fwd_gnbwd_blocks(...) (0: shape not taken; use diqt_conv3d_fwd + diqt_gn_act_bwd).
 * diqt_gn_act_bwd_from_partials then finishes the GroupNorm backward without its own reduction pass over x and dy.
 * Replaces autograd of Block.forward (imagen_pytorch3D.py:535-566, imagen_video.py:671-697).                                       */
int diqt_conv3d_fwd_gnbwd_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd,
                                 int eph, int epw);
/* Block.forward on the sampling path as one launch (GroupNorm -> (scale + 1) x + shift -> Mish / SiLU -> conv;
 * imagen_pytorch3D.py:546-566, imagen_video.py:680-697): diqt_gn_coef_from_partials (statistics from the producer's column sums) or
 * diqt_gn_coef (from existing statistics) fold the normalisation into y = act(A x + Bc), coef[2][B][C] = (A, Bc); diqt_conv3d_fwd_gn
 * takes the RAW GroupNorm input x and applies the coefficients while it stages its input tiles (arguments otherwise as
 * diqt_conv3d_fwd_ex).  diqt_conv3d_fwd_gn_supported = 0: use diqt_gn_act_fwd + diqt_conv3d_fwd_ex.  act: DIQT_ACT_MISH on 3x3x3
 * filters, DIQT_ACT_SILU on (1,3,3) filters.  `stats`: the rows diqt_conv3d_fwd_route grants this ask (gn_act = act, field 3) -- those
 * of diqt_conv3d_fwd_stats_blocks* where the launch runs un-split, none where it splits K.                                         */
int diqt_gn_coef_from_partials(const float* partials, int nblk, int rows, const float* gamma, const float* beta, const float* scale,
                               const float* shift, int cond_stride, float* mean, float* rstd, float* coef, int B, int C, int G,
                               float eps, void* stream);
int diqt_groupnorm_stats_coef(const float* x, const float* gamma, const float* beta, const float* scale, const float* shift,
                              int cond_stride, float* mean, float* rstd, float* coef, void* workspace, size_t workspace_bytes, int B,
                              int rows, int C, int G, float eps, void* stream);      /* diqt_groupnorm_stats + the coefficients */
int diqt_gn_coef(const float* mean, const float* rstd, const float* gamma, const float* beta, const float* scale, const float* shift,
                 int cond_stride, float* coef, int B, int C, int G, void* stream);
int diqt_conv3d_fwd_gn_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd,
                                 int eph, int epw, int act);
int diqt_conv3d_fwd_gn(const float* x, const float* packed, const float* bias, const float* residual, float* y, float* stats,
                       void* workspace, size_t workspace_bytes, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout,
                       int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream);
/* the same told the length of the packed buffer, as diqt_conv3d_fwd_pk (Winograd tile with Mish on the 3x3x3 launches) */
int diqt_conv3d_fwd_gn_supported_pk(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                    int epd, int eph, int epw, int act, size_t packed_elems);
int diqt_conv3d_fwd_gn_pk(const float* x, const float* packed, size_t packed_elems, const float* bias, const float* residual, float* y,
                          float* stats, void* workspace, size_t workspace_bytes, const float* coef, int act, int B, int D, int H,
                          int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw,
                          void* stream);

/* Process-wide switch of that fusion (default: off unless DIQT_GNBWD_FUSE=1 in the environment at the first query).  The setter
 * returns the previous value; with the switch off diqt_conv3d_fwd_gnbwd_blocks answers 0 for every shape.  Host-side state only
 * (no reference counterpart: both settings compute autograd of Block.forward, imagen_pytorch3D.py:535-566).                        */
int diqt_get_gnbwd_fuse(void);
int diqt_set_gnbwd_fuse(int on);
int diqt_conv3d_fwd_gnbwd(const float* x, const float* packed, float* y, float* partials, const float* gn_x, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, const float* scale, const float* shift,
                          int cond_stride, int G, int act, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd,
                          int ph, int pw, int epd, int eph, int epw, void* stream);
/* As diqt_gn_act_bwd (partials == NULL) / diqt_gn_act_bwd_from_partials, plus dx_add (optional, same shape as x): dx = GroupNorm
 * backward + dx_add -- the gradient that reaches x through its second consumer (ResnetBlock: x feeds block1 AND the residual branch,
 * imagen_pytorch3D.py:601-614, imagen_video.py:745-770), so the framework's separate sum over the two branches disappears.          */
int diqt_gn_act_bwd_ex(const float* x, const float* dy, const float* partials, int nblk, const float* dx_add, const float* mean,
                       const float* rstd, const float* gamma, const float* beta, const float* scale, const float* shift,
                       int cond_stride, float* dx, float* dgamma, float* dbeta, float* dscale, float* dshift, void* workspace,
                       size_t workspace_bytes, int B, int rows, int C, int G, int act, void* stream);
/* diqt_gn_act_bwd_ex with x / dy read and / or dx written in a 16-bit type (x_type, dx_type, dy_type: 0 fp32, 1 fp16, 2 bf16): the block1
 * output of a ResnetBlock and the gradient flowing back into it during a low-precision training step (both only meet 16-bit-operand
 * kernels); dy: the output of the backward-data conv in front of this pass, which autocast's backward holds in the operand type. */
int diqt_gn_act_bwd_h(const void* x, const void* dy, const float* partials, int nblk, const float* dx_add, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, const float* scale, const float* shift, int cond_stride,
                      void* dx, float* dgamma, float* dbeta, float* dscale, float* dshift, void* workspace, size_t workspace_bytes, int B,
                      int rows, int C, int G, int act, int x_type, int dx_type, int dy_type, void* stream);
int diqt_gn_act_bwd_from_partials(const float* x, const float* dy, const float* partials, int nblk, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, const float* scale, const float* shift, int cond_stride,
                                  float* dx, float* dgamma, float* dbeta, float* dscale, float* dshift, void* workspace,
                                  size_t workspace_bytes, int B, int rows, int C, int G, int act, void* stream);

/* Per-position LayerNorm over the channel axis, biased variance; gain `g` and optional bias `b` (NULL for the
 * gain-only ChanLayerNorm imagen_pytorch3D.py:361-382 / LayerNorm imagen_video.py:172-200; non-NULL for
 * nn.LayerNorm at imagen_video.py:444,1306).                                                           */
int diqt_chan_layernorm_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd,
                            int rows, int C, float eps, void* stream);
/* The same with `+ residual` in the same pass: Residual(Attention) / TransformerBlock `attn(x) + x`, whose to_out ends in a LayerNorm
 * (imagen_video.py:217-224, 483-525, 1004-1029); residual may be NULL.                                                          */
int diqt_chan_layernorm_fwd_res(const float* x, const float* g, const float* b, const float* residual, float* y, float* mean,
                                float* rstd, int rows, int C, float eps, void* stream);

/* Depthwise temporal conv of the pseudo-3D U-Net's TemporalPEG -- nn.Conv3d(C, C, (3,1,1), groups=C) after a causal (2,0) or symmetric
 * (1,1) frame pad, wrapped in a Residual (/root/reference/imagen_video.py:1340-1362): x[B][F][P][C] channels-last, w[C][kt], kt = 3,
 * `left` frames of zero padding in front.  y = conv(x) + bias (+ residual).  flip = 1 with left' = kt - 1 - left is the gradient
 * w.r.t. x.  The weight gradient comes tap-major with the bias gradient as its last row: dwb[kt + 1][C].                          */
int diqt_dwconv_temporal_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int F, int P,
                             int C, int kt, int left, int flip, void* stream);
size_t diqt_dwconv_temporal_bwd_weight_workspace_bytes(int B, int F, int P, int C, int kt);
int diqt_dwconv_temporal_bwd_weight(const float* x, const float* dy, float* dwb, void* workspace, size_t workspace_bytes, int B, int F,
                                    int P, int C, int kt, int left, void* stream);

/* dg[C], db[C] (db may be NULL) are reduced through `workspace` (diqt_reduce_workspace_bytes(1, C)) */
int diqt_chan_layernorm_bwd(const float* x, const float* dy, const float* g, const float* mean,
                            const float* rstd, float* dx, float* dg, float* db, void* workspace,
                            size_t workspace_bytes, int rows, int C, void* stream);
/* ... plus dx_add (optional, same shape as x): dx = LayerNorm backward + dx_add, the residual branch's gradient of `fn(LN(x)) + x`
 * (Attention / ChanFeedForward blocks, imagen_video.py:410-525, 994-1029) summed in the same pass.  With dg the workspace must be
 * 16-byte aligned, and with db and C % 4 == 0, C <= 1024 so must dy (DIQT_E_ALIGN otherwise, nothing launched).                       */
int diqt_chan_layernorm_bwd_ex(const float* x, const float* dy, const float* dx_add, const float* g, const float* mean,
                               const float* rstd, float* dx, float* dg, float* db, void* workspace,
                               size_t workspace_bytes, int rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise activations (n floats) — nn.Mish / SiLU / GELU / ReLU / Sigmoid call sites above.
 * ---------------------------------------------------------------------------------------------- */
int diqt_act_fwd(const float* x, float* y, size_t n, int act, void* stream);
int diqt_act_bwd(const float* x, const float* dy, float* dx, size_t n, int act, void* stream);

/* Skinny nn.Linear for the time-conditioning MLPs (imagen_pytorch3D.py:589-606 to_time_hiddens / to_time_cond /
 * to_time_tokens, :554-557 ResnetBlock.time_mlp; imagen_video.py:1226-1262): y[M][N] = x[M][K] W[N][K]^T + bias,
 * 0 < M <= 64 (batch rows).  W is the nn.Linear [out][in] layout.  bias may be NULL.                    */
int diqt_linear_small_fwd(const float* x, const float* W, const float* bias, float* y, int M, int K, int N, void* stream);
/* dx[M][K], dw[N][K], db[N] (each may be NULL; db needs dw).  dx goes through `workspace`.             */
size_t diqt_linear_small_workspace_bytes(int M, int K, int N);
int diqt_linear_small_bwd(const float* x, const float* W, const float* dy, float* dx, float* dw, float* db,
                          void* workspace, size_t workspace_bytes, int M, int K, int N, void* stream);

/* LearnedSinusoidalPosEmb (imagen_pytorch3D.py:518-533): out[b] = [t, sin(2 pi t w), cos(2 pi t w)] */
int diqt_learned_sinu_fwd(const float* t, const float* w, float* out, int B, int half, void* stream);
/* dw[half] (overwritten) from dout[B][2*half+1] */
int diqt_learned_sinu_bwd(const float* t, const float* w, const float* dout, float* dw, int B, int half, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Squeeze-excite + residual — SE3D imagen_pytorch3D.py:617-632 and `h + res_conv(x)` :610-612.
 * ---------------------------------------------------------------------------------------------- */
/* pooled[b][c] = mean over rows_per_batch of x[b][.][c]  (AdaptiveAvgPool3d(1) :620,630) */
int diqt_channel_mean(const float* x, float* pooled, void* workspace, size_t workspace_bytes,
                      int B, int rows_per_batch, int C, void* stream);
/* The whole pooling of GlobalContext in one pass over x (sampling path): pooled[b][c] = sum_n softmax_n(x[b][n][:] . w)[n] * x[b][n][c]
 * -- to_k (a 1x1 conv to one channel; its bias drops out of the soft-max), softmax over all positions and the weighted sum
 * (imagen_video.py:957-982).  Online soft-max, fixed-order combines.  C in {64, 128, 256}; workspace: diqt_reduce_workspace_bytes(B, C). */
int diqt_softmax_pool_supported(int B, int rows, int C);
int diqt_softmax_pool(const float* x, const float* w, float* pooled, void* workspace, size_t workspace_bytes, int B, int rows, int C,
                      void* stream);
/* out[b][c] = sum_rows w[b][row] * x[b][row][c] — the attention-weighted pooling of GlobalContext
 * (imagen_video.py:975-979: einsum('b i n, b c n -> b c i', softmax(context), x)); workspace: diqt_reduce_workspace_bytes(B, C). */
int diqt_weighted_colsum(const float* x, const float* w, float* out, void* workspace, size_t workspace_bytes,
                         int B, int rows, int C, void* stream);

/* y = h*gate[b][c] + res + alpha*addc[b][c]   (res, addc may be NULL).  The same entry yields the
 * backward dh = dy*gate + (1/rows)*dpooled[b][c] of the gate AND of the mean pool in one pass.        */
int diqt_gate_residual_fwd(const float* h, const float* gate, const float* res, const float* addc, float alpha,
                           float* y, int B, int rows_per_batch, int C, void* stream);
/* The same with res only, plus per-workgroup column sums of y for the consumer's GroupNorm statistics (a ResnetBlock's output feeds
 * the next block's first GroupNorm, imagen_pytorch3D.py:568-614): stats[B][nblk][2 (sum, sum of squares)][C],
 * nblk = diqt_gate_residual_stats_blocks(rows, C) (0: C is not a multiple of 4 dividing 1024 -- use the plain entry point).
 * Feed them to diqt_groupnorm_stats_from_partials; saves one full read of y.                                                  */
int diqt_gate_residual_stats_blocks(int rows, int C);
int diqt_gate_residual_fwd_stats(const float* h, const float* gate, const float* res, float* y, float* stats, int B, int rows, int C,
                                 void* stream);
/* dgate[b][c] = sum_rows dy*h */
int diqt_gate_residual_bwd(const float* h, const float* dy, float* dgate, void* workspace, size_t workspace_bytes,
                           int B, int rows_per_batch, int C, void* stream);
/* The SE gate with the conv output h and the gradient flowing back into it in a 16-bit type (h_type / y_type: 0 fp32, 1 fp16, 2 bf16): a
 * ResnetBlock's block2 output under autocast sampling / low-precision training exists in the operand type only -- autocast rounds a conv
 * result to it anyway (imagen_pytorch3D.py:601-632).  _fwd_h: y = h gate (+ res) (+ alpha addc[b][c]); with res = NULL and addc it is also
 * the backward dh = dy gate + dpooled / rows, written in y_type.                                                                       */
int diqt_gate_residual_fwd_h(const void* h, const float* gate, const float* res, const float* addc, float alpha, void* y, int B, int rows,
                             int C, int h_type, int y_type, void* stream);
int diqt_gate_residual_fwd_stats_h(const void* h, const float* gate, const float* res, float* y, float* stats, int B, int rows, int C,
                                   int h_type, void* stream);
int diqt_gate_residual_bwd_h(const void* h, const float* dy, float* dgate, void* workspace, size_t workspace_bytes, int B, int rows, int C,
                             int h_type, void* stream);
/* SE3D.fc (imagen_pytorch3D.py:621-626,631): hidden = relu(pooled w1^T), gate = sigmoid(hidden w2^T);
 * w1[Cr][C], w2[C][Cr], no biases.  bwd: dpooled, dw1, dw2 from dgate; scratch >= B*(C+Cr) floats.     */
int diqt_se_mlp_fwd(const float* pooled, const float* w1, const float* w2, float* hidden, float* gate,
                    int B, int C, int Cr, void* stream);
/* SE3D squeeze + excitation in ONE launch, one workgroup per batch entry: the channel means are finished from the producer's
 * per-tile column sums `partials` [B][nblk][2][C] (diqt_conv3d_fwd_ex) -- or read from `pooled` when partials == NULL -- then
 * fc1 -> ReLU -> fc2 -> sigmoid.  Writes pooled (when computed here), hidden [B][Cr] and gate [B][C].                         */
int diqt_se_pool_mlp_fwd(const float* partials, int nblk, int rows, float* pooled, const float* w1, const float* w2, float* hidden,
                         float* gate, int B, int C, int Cr, void* stream);
int diqt_se_mlp_bwd(const float* pooled, const float* w1, const float* w2, const float* hidden, const float* gate,
                    const float* dgate, float* dpooled, float* dw1, float* dw2, float* scratch,
                    int B, int C, int Cr, void* stream);
/* x[b][.][c] += v[b][c] broadcast (backward of the mean pool, scaled by caller) and friends */
int diqt_add_channel_broadcast(float* x, const float* v, float alpha, int B, int rows_per_batch, int C,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data movement — Downsample rearrange imagen_pytorch3D.py:494, PixelShuffle3D :427-439,
 * torch.cat on channels :1576,1653, sub-volume split/merge utils_mine.py:25-67, halo :37-46.
 * ---------------------------------------------------------------------------------------------- */
/* x[B][2D][2H][2W][C] -> y[B][D][H][W][C*8], out channel = c*8 + s1*4 + s2*2 + s3 */
int diqt_space_to_depth2(const float* x, float* y, int B, int D, int H, int W, int C, void* stream);
/* exact inverse (x[B][D][H][W][C*8] -> y[B][2D][2H][2W][C]); also PixelShuffle3D(2) forward */
int diqt_depth_to_space2(const float* x, float* y, int B, int D, int H, int W, int C, void* stream);
/* generic factor-(sd,sh,sw) version, each factor 1 or 2 (2-D per-frame shuffles of imagen_video.py:564-600:
 * Rearrange 'b c f (h p1) (w p2) -> b (c p1 p2) f h w' and nn.PixelShuffle(2)); D,H,W are the coarse extents */
int diqt_space_to_depth_nd(const float* x, float* y, int B, int D, int H, int W, int C, int sd, int sh, int sw, void* stream);
int diqt_depth_to_space_nd(const float* x, float* y, int B, int D, int H, int W, int C, int sd, int sh, int sw, void* stream);
/* x[A][M][N][C] -> y[A][N][M][C]  ('b c f h w' <-> '(b h w) f c' token views, imagen_video.py:1354) */
int diqt_transpose_mid(const float* x, float* y, int A, int M, int N, int C, void* stream);
/* F.interpolate(mode='nearest') on channels-last volumes (resize_video_to imagen_video.py:137-158) */
int diqt_nearest_resize(const float* x, float* y, int B, int D, int H, int W, int C, int Do, int Ho, int Wo, void* stream);
/* its gradient for whole-number up-scaling factors (UpsampleCombiner's resize_video_to of the up-path feature maps,
 * imagen_video.py:1085-1117): dx[b][d][h][w][c] = sum of the Do/D x Ho/H x Wo/W copies in dy                                       */
int diqt_nearest_resize_bwd(const float* dy, float* dx, int B, int D, int H, int W, int C, int Do, int Ho, int Wo, void* stream);
/* F.normalize(dim = -1) over rows of d floats (the l2norm of cosine-sim attention, imagen_video.py:118-119, 484-486, 828-829): rows of
 * x are x_stride floats apart (so the k half of a [.., 2d] k|v row can be normalised in place of a copy), rows of y / dy / dx
 * y_stride / dx_stride apart; inv[rows] = 1 / max(||x||, 1e-12) is kept for the backward dx = (dy - y (y . dy)) inv.               */
int diqt_l2norm_rows_fwd(const float* x, float* y, float* inv, size_t rows, int d, int x_stride, int y_stride, void* stream);
int diqt_l2norm_rows_bwd(const float* y, const float* dy, const float* inv, float* dx, size_t rows, int d, int y_stride, int dx_stride,
                         void* stream);
/* y[rows][Ca+Cb] = cat(a[rows][Ca], b[rows][Cb]) ; and the inverse split */
int diqt_concat_channels(const float* a, int Ca, const float* b, int Cb, float* y, size_t rows, void* stream);
int diqt_split_channels(const float* y, float* a, int Ca, float* b, int Cb, size_t rows, void* stream);
/* y = cat(sa * a, sb * b) over the channel axis and its adjoint (a = sa * y[:, :Ca], b = sb * y[:, Ca:]; either output may be NULL):
 * the scaled skip connections cat(x, skip * 2^-0.5) of the U-Nets (imagen_video.py:1743, imagen_pytorch3D.py:1631) in one pass.
 * float4 lanes when both channel counts are multiples of 4.                                                                  */
int diqt_concat_channels_scaled(const float* a, int Ca, const float* b, int Cb, float sa, float sb, float* y, size_t rows, void* stream);
/* The same pass ALSO writing the column sums (sum, sum of squares) of y per 256-row block, stats[B][nblk][2][Ca + Cb] with nblk =
 * diqt_concat_channels_stats_blocks (0: shape not taken): the concatenated skip connection feeds a ResnetBlock's GroupNorm
 * (imagen_video.py:1743-1747, imagen_pytorch3D.py:1631-1633), whose statistics then come from diqt_groupnorm_stats_from_partials. */
int diqt_concat_channels_stats_blocks(int Ca, int Cb, int rows_per_batch);
int diqt_concat_channels_stats(const float* a, int Ca, const float* b, int Cb, float sa, float sb, float* y, int B, int rows_per_batch,
                               float* stats, void* stream);
int diqt_split_channels_scaled(const float* y, float* a, int Ca, float* b, int Cb, float sa, float sb, size_t rows, void* stream);
/* trilinear x`scale` up-sampling with align_corners=True (nn.Upsample imagen_pytorch3D.py:954) and its
 * adjoint (dx must be zeroed by the caller; accumulated with float atomics)                          */
int diqt_trilinear_up_fwd(const float* x, float* y, int B, int D, int H, int W, int C, int scale, void* stream);
int diqt_trilinear_up_bwd(const float* dy, float* dx, int B, int D, int H, int W, int C, int scale, void* stream);
/* sub-volume batch <-> merged volume, NDHWC; sub-volume n = b2 + f*b3 + f*f*b4 (utils_mine.py:41).
 * halo>0 gathers (A+2*halo)^3 blocks from the zero-padded merged volume (boundary_pad).             */
int diqt_subvolume_gather(const float* vol, float* sub, int f, int A, int C, int halo, void* stream);
int diqt_subvolume_scatter(const float* sub, float* vol, int f, int A, int C, int halo, int accumulate,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diffusion elementwise steps.
 * ---------------------------------------------------------------------------------------------- */
/* x_t = alpha[b]*x0 + sigma[b]*noise   — q_sample imagen_pytorch3D.py:311-322 */
int diqt_q_sample(const float* x0, const float* noise, const float* alpha, const float* sigma,
                  float* xt, int B, size_t per_batch, void* stream);
/* DDPM ancestral step — p_mean_variance/p_sample imagen_pytorch3D.py:1996-2055, q_posterior :290-309.
 * x0 = clamp(pred) [clamp_mode 0: min=lo ; 1: [lo,hi]]; x_next = ca[b]*x_t + cb[b]*x0 + cn[b]*noise,
 * where the caller precomputes ca = alpha_next*(1-c)/alpha, cb = alpha_next*c, cn = nonzero*exp(.5*logvar). */
int diqt_ddpm_step(const float* x_t, const float* pred, const float* noise,
                   const float* ca, const float* cb, const float* cn, float lo, float hi, int clamp_mode,
                   float* x_next, float* x0_out, int B, size_t per_batch, void* stream);
/* generic per-batch affine combination used by the EDM Heun sampler (elucidated_imagen.py:476-516):
 * out = clamp( c0[b]*a + c1[b]*b_ + c2[b]*c_ ) ; b_/c_ may be NULL; clamp_mode 0 none, 1 min=lo, 2 [lo,hi] */
int diqt_axpby3(const float* a, const float* b_, const float* c_, const float* c0, const float* c1,
                const float* c2, float lo, float hi, int clamp_mode, float* out,
                int B, size_t per_batch, void* stream);
/* loss = mean_b mean_i (clamp_min(pred,lo) - target)^2, per-batch weights w[b] (NULL = 1)
 * — p_losses imagen_pytorch3D.py:2361-2364; the clamped prediction the reference returns is written to
 * pred_clamped (may alias pred for the reference's in-place form, or be NULL).
 * loss_out: single float (atomic-free two-stage reduce through `partials`, >= 1024 floats).          */
/* diqt_mse_clamp_fwd / _bwd with the per-element loss selected by `kind`: 0 squared error (F.mse_loss), 1 absolute error (F.l1_loss),
 * 2 Huber with beta 1 (F.smooth_l1_loss) -- Imagen(loss_type = 'l2' | 'l1' | 'huber'), imagen_pytorch3D.py:1785-1790, 2370.        */
int diqt_loss_clamp_fwd(const float* pred, float* pred_clamped, const float* target, const float* w, float lo, int do_clamp, int kind,
                        float* partials, float* loss_out, int B, size_t per, void* stream);
int diqt_loss_clamp_bwd(const float* pred, const float* target, const float* w, float lo, int do_clamp, int kind, float gscale,
                        float* dpred, int B, size_t per, void* stream);
int diqt_mse_clamp_fwd(const float* pred, float* pred_clamped, const float* target, const float* w, float lo,
                       int do_clamp, float* partials, float* loss_out, int B, size_t per_batch, void* stream);
/* dpred = gscale * 2*(pred-target)*w[b]/(B*per_batch), zero where pred was clamped (pred <= lo)      */
int diqt_mse_clamp_bwd(const float* pred_clamped, const float* target, const float* w, float lo,
                       int do_clamp, float gscale, float* dpred, int B, size_t per_batch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser — Adam (trainer.py:352-359, step at :1056) fused with zero_grad, and the EMA lerp
 * (ema_pytorch, trainer.py:1059-1061), over one flat fp32 arena.
 * ---------------------------------------------------------------------------------------------- */
int diqt_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_correction1, float bias_correction2, int zero_grad, void* stream);
/* Global gradient-norm clipping (ImagenTrainer(max_grad_norm=...): accelerator.clip_grad_norm_ -> torch.nn.utils.clip_grad_norm_,
 * trainer.py:1054) over the flat gradient arena.  diqt_grad_norm_clip writes out2[0] = L2 norm of grad[0..n) (fixed-order, fp64
 * combine) and out2[1] = min(1, max_norm / (norm + 1e-6)); `workspace`: diqt_grad_norm_workspace_bytes() bytes, 8-byte aligned.
 * diqt_adam_step_scaled is diqt_adam_step with every gradient multiplied by *grad_scale (a device scalar, e.g. out2 + 1) first. */
size_t diqt_grad_norm_workspace_bytes(void);
int diqt_grad_norm_clip(const float* grad, size_t n, float max_norm, void* workspace, float* out2, void* stream);
int diqt_adam_step_scaled(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                          float lr, float beta1, float beta2, float eps, float weight_decay,
                          float bias_correction1, float bias_correction2, int zero_grad, const float* grad_scale, void* stream);
/* Dynamic thresholding of the predicted x0 (imagen_pytorch3D.py:2006-2021; elucidated_imagen.py:340-358):
 * out[b] = torch.quantile(|x[b, :]|, q) with linear interpolation.  The caller passes the fp32 rank split the way
 * torch does: rank = q * (per - 1) in fp32, k_lo = floor(rank), weight = rank - k_lo.                              */
int diqt_abs_quantile(const float* x, float* out, int B, size_t per_batch, unsigned k_lo, float weight, void* stream);
/* out = clamp(x0, -s[b], s[b]) / s[b] */
int diqt_dynamic_threshold(const float* x0, const float* s, float* out, int B, size_t per_batch, void* stream);
/* Inpainting blend (imagen_pytorch3D.py:2121-2123): out = mask != 0 ? y : x  (mask as 0/1 floats, n elements) */
int diqt_mask_blend(const float* x, const float* y, const float* mask, float* out, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-volume inference (test_all.py:182-300 with data.py:138-202): sliding-window patches of a volume resident in HBM.
 * `idx` = int32 [n][3] patch origins; volumes are fp32 [D][H][W].
 * ---------------------------------------------------------------------------------------------- */
/* out[n][P][P][P] = (vol[origin + ijk] - mean) / std (out may be NULL); nonzero[n] = non-zero RAW voxels (may be NULL):
 * supervisedIQT_INF.__getitem__ / normalize (data.py:168-199) incl. its 5 % non-zero rejection count.               */
int diqt_patch_gather(const float* vol, const int* idx, float* out, int* nonzero, int n_patches, int D, int H, int W, int P,
                      float mean, float stdv, void* stream);
/* pred[origin + ijk] = patches[n][ijk] inside the crop margins[n] = {lo_i, hi_i, lo_j, hi_j, lo_k, hi_k}
 * (the overlap//2 crop with edge special cases, test_all.py:235-298).  Patches are written in index order per launch;
 * overlapping writes of one launch must carry equal margins-free regions (the caller launches overlapping blocks one by one). */
int diqt_patch_scatter(const float* patches, const int* idx, const int* margins, float* pred, int n_patches, int D, int H, int W,
                       int P, void* stream);
/* pred[i] = min_val where (vol[i] - mean) / std == min_val (test_all.py:300) */
int diqt_background_reset(float* pred, const float* vol, size_t n, float mean, float stdv, float min_val, void* stream);
/* out[0] = min(x[0..n)); workspace: 1024 floats */
int diqt_min_value(const float* x, size_t n, float* workspace_1024, float* out, void* stream);
/* Weighted overlap blending, in place of the crop-and-overwrite stitching and the background reset of test_all.py:235-300:
 * patches[S][N][P][P][P] holds S samples of the N kept windows in candidate order; slot[G0][G1][G2] (G_a =
 * len(range(0, n_a - P + 1, stride))) is a window's row in `patches`, or < 0 for one that was not kept; taps[P] (DEVICE) is the
 * 1-D window.  Per output voxel and sample, over the covering windows in candidate order: b_s = sum(w y) / sum(w) with
 * w = (taps[i] taps[j]) taps[k]; out_mean = mean of b_s, out_std (may be NULL; must be NULL when S == 1) = their unbiased standard
 * deviation (Welford, sample order).  A voxel no kept window covers gets `fill` (deviation 0); where vol (RAW, may be NULL) has
 * (vol - mean) / std == min_val the voxel gets min_val (deviation 0).  One launch, gather-side, no atomics: bit-reproducible.   */
int diqt_volume_blend(const float* patches, const int* slot, const float* taps, const float* vol, float* out_mean, float* out_std,
                      int S, int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2, float mean, float stdv,
                      float min_val, float fill, void* stream);
/* Volume-anchored sampler noise: out[b][c][i][j][k] for the B windows origins[b] = {z0, y0, x0} (int32, DEVICE) of edge P inside a
 * C-channel [D][H][W] volume is a pure function of (seed, c, z0 + i, y0 + j, x0 + k, draw, sample) -- every window that covers a voxel
 * gets the same number, whatever batch or order it arrives in.  Per voxel: lin = ((c D + z) H + y) W + x as an unsigned 64-bit
 * integer; ONE Philox4x32-10 call (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds) with
 * counter {lin & 0xffffffff, lin >> 32, draw, sample} and key {seed & 0xffffffff, seed >> 32}; output words r0, r1 are used, r2, r3
 * dropped.  raw = 1: out is int32 [B][C][P][P][P][2] = {r0, r1}.  raw = 0: out is fp32 [B][C][P][P][P], the Box-Muller normal
 * n = sqrtf(-2 logf(u1)) cospif(2 u2) with u1 = ((r0 >> 9) + 0.5) 2^-23 in (0, 1) and u2 = (r1 >> 8) 2^-24 (both exact in fp32).
 * The caller guarantees that every window lies inside the volume (the origins are on the device; the entry cannot look at them). */
int diqt_anchored_noise(const int* origins, int B, int C, int P, int D, int H, int W, unsigned long long seed, unsigned draw,
                        unsigned sample, int raw, void* out, void* stream);
/* Lockstep joint sampling of the overlapping windows (MultiDiffusion, Bar-Tal et al. 2023): ONE reverse step of the noisy state of the
 * whole [D][H][W] volume.  y[N][P][P][P] holds the kept windows' x0 predictions of this step in candidate order; slot / taps (DEVICE) /
 * stride / G* are diqt_volume_blend's, with the same lattice check.  Per output voxel, over the covering kept windows in candidate
 * order: num = fma(w, c(y), num), den += w with w = (taps[i] taps[j]) taps[k] and c the clamp of diqt_ddpm_step (clamp_mode 0:
 * max(y, lo); 1: min(max(y, lo), hi)) -- diqt_volume_blend's arithmetic for S = 1.  Covered voxel (den != 0): x0 = num / den,
 * x_next = kx x_t + k0 x0 + kn n in diqt_ddpm_step's operation order, n = the normal of diqt_anchored_noise for channel 0 at (seed,
 * z, y, x, draw, sample), or 0 when kn == 0; x0_out (may be NULL) = x0.  Uncovered voxel: x_next = x_t, x0_out = 0.  x_next may alias
 * x_t.  x_t == NULL is the initial state: x_next = that normal of `draw` at EVERY voxel, bit for bit diqt_anchored_noise's, and the
 * window arguments (y, slot, taps, x0_out, N, P, stride, G*, the coefficients and the clamp) are ignored.  One launch, gather-side,
 * no atomics: bit-reproducible.                                                                                                  */
int diqt_volume_joint_step(const float* y, const int* slot, const float* taps, const float* x_t, float* x_next, float* x0_out, int N,
                           int D, int H, int W, int P, int stride, int G0, int G1, int G2, float kx, float k0, float kn, float lo,
                           float hi, int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* One step of a second-order multistep chain (DPM-Solver++ 2M; Lu et al. 2022) on the joint state: diqt_volume_joint_step with the
 * fused x0 of the PREVIOUS step as the third operand instead of a normal -- no Philox, no seed, no draw.  Window walk, clamp, lattice
 * check and launch geometry are diqt_volume_joint_step's.  Covered voxel (den != 0): x0 = num / den and
 *     b = k0 * x0;  c = kp * x0_prev[v];  x_next[v] = fmaf(kx, x_t[v], b) + c
 * with b and c rounded products (no further contraction) -- diqt_ddpm_step's operation order with x0_prev in the place of its noise
 * operand; x0_out[v] = x0.  Uncovered voxel: x_next = x_t, x0_out = 0.  x0_prev == NULL stands for zeros (the first step).  x_next
 * may alias x_t and x0_out may alias x0_prev: every thread reads its own voxel of both before it writes it.  x0_out is required.
 * With kp == 0 and x0_prev == NULL, x_next and x0_out are bit for bit diqt_volume_joint_step's at kn == 0.  Null pointers:
 * DIQT_E_ALIGN; a lattice that does not match: DIQT_E_SHAPE; clamp_mode outside {0, 1}: DIQT_E_UNSUPPORTED.                       */
int diqt_volume_joint_multistep(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                float* x_next, float* x0_out, int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2,
                                float kx, float k0, float kp, float lo, float hi, int clamp_mode, void* stream);
/* DPM-Solver++ 2M in sigma space for the EDM family (ElucidatedImagen(sampler='dpmpp2m')), ODE and midpoint SDE: one step of ONE window
 * batch, in place of the diqt_axpby3 sequence of a Heun step (two U-Net evaluations, three or four launches).  x / x0 / x0_prev / noise
 * are [B][per_batch], kx / k0 / kp / kn DEVICE [B] (one coefficient row per sample):
 *     b = k0 * x0;  c = kp * x0_prev;  u = fmaf(kx, x, b) + c;  if (kn != 0) u = u + kn * noise
 * with b, c and kn * noise rounded products (no further contraction) -- diqt_volume_joint_multistep's update, then the noise term last.
 * x0_prev == NULL and noise == NULL stand for zeros and are not read; noise is not read for a sample whose kn is 0.  There is no
 * clamp (x0 arrives clamped or thresholded).  x_next may alias x.  Null pointers: DIQT_E_ALIGN; B <= 0, per_batch == 0 or B > 65535:
 * DIQT_E_SHAPE.                                                                                                                   */
int diqt_multistep_sde_step(const float* x, const float* x0, const float* x0_prev, const float* noise, const float* kx, const float* k0,
                            const float* kp, const float* kn, float* x_next, int B, size_t per_batch, void* stream);
/* The same step on the joint state, in place of diqt_volume_joint_heun's two phases per step: diqt_volume_joint_multistep plus the
 * volume-anchored normal n of diqt_volume_joint_step (channel 0 at (seed, z, y, x, draw, sample)).  Covered voxel: x0 = num / den and
 * the update of diqt_multistep_sde_step with that n (no Philox call when kn == 0, and then x_next and x0_out are bit for bit
 * diqt_volume_joint_multistep's); x0_out = x0.  Uncovered voxel: x_next = x_t, x0_out = 0.  x_t == NULL is the initial state:
 * x_next = kn * n(draw) at EVERY voxel (one rounded product: the initial image sigma0 n as the per-window sampler stores it), and the
 * window arguments, x0_prev, x0_out, the other coefficients and the clamp are ignored.  x_next may alias x_t and x0_out may alias
 * x0_prev.  Error codes are diqt_volume_joint_multistep's.                                                                          */
int diqt_volume_joint_multistep_sde(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                    float* x_next, float* x0_out, int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2,
                                    float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode, unsigned long long seed,
                                    unsigned draw, unsigned sample, void* stream);
/* Data-consistent sampling for a block-average measurement (DDNM; Wang, Yu, Zhang, ICLR 2023).  A cell is (fz, fy, fx) voxels, every
 * factor >= 1 and n = fz fy fx in 2 .. 64; voxel (z, y, x) belongs to cell (z / fz, y / fy, x / fx).  The measurement is the cell mean
 * (the operator A) and the kernels read it REPLICATED on the high-res grid: meas_up[v] = the measurement of v's cell (A+ applied to
 * it).  The projection of the values a over one cell, in fp32 with no contraction, ONE definition for every entry below:
 *     s = 0;  s = s + a[v] over the cell's voxels in lexicographic (z, y, x) order;  m = s / (float)n;
 *     a'[v] = fmaf(w, meas_up[v] - m, a[v])     for every voxel of the cell, w the consistency weight, 0 < w <= 1
 * (w = 1: x0' = x0 + A+(y - A x0), the cell means land on the measurement and the detail inside a cell is untouched; w < 1: DDNM's
 * relaxation for a noisy measurement).  Error codes shared by the three entries: a null pointer: DIQT_E_ALIGN; a cell with a factor
 * < 1 or n outside 2 .. 64, or w outside (0, 1]: DIQT_E_UNSUPPORTED; an extent the cell does not divide: DIQT_E_SHAPE.
 *
 * diqt_cell_mean: out [D / fz][H / fy][W / fx] = m of x [D][H][W] -- A itself, to simulate a measurement.  out may not alias x.     */
int diqt_cell_mean(const float* x, float* out, int D, int H, int W, int fz, int fy, int fx, void* stream);
/* The per-window step: x0 / meas_up / out hold `cubes` cubes of edge P ([B][C P^3]: B C cubes).  a = c(x0) with c the clamp of
 * diqt_ddpm_step (clamp_mode 0: max(x0, lo); 1: min(max(x0, lo), hi)) or, clamp_mode 2, the identity; then the projection.  The clamp
 * belongs here because the projection must come after it: the step that follows takes the result unclamped.  out may alias x0 (a
 * thread reads and writes the voxels of its own cells only); meas_up may not alias out.  P % fz, P % fy or P % fx != 0 or cubes == 0:
 * DIQT_E_SHAPE; clamp_mode outside {0, 1, 2}: DIQT_E_UNSUPPORTED.                                                                  */
int diqt_cell_project(const float* x0, const float* meas_up, float* out, size_t cubes, int P, int fz, int fy, int fx, float weight,
                      float lo, float hi, int clamp_mode, void* stream);
/* The three linear updates of the joint state with the projection between the fuse and the update; meas_up is [D][H][W] in state
 * space.  `form`, uniform over the launch: 0 = diqt_volume_joint_step (x0_prev and kp are ignored), 1 = diqt_volume_joint_multistep
 * (kn, seed, draw and sample are ignored), 2 = diqt_volume_joint_multistep_sde.  Window walk, clamp, lattice check, the normals and
 * the update of each form are that entry's.  Per cell: every voxel is fused as there, x0 = num / den under the step clamp.  A cell
 * whose voxels are ALL covered (den != 0) takes the projection of its fused x0, and each of its voxels the form's update with x0' in
 * the place of x0.  A cell with an uncovered voxel is left alone: its covered voxels take the update with their plain x0, its
 * uncovered voxels keep x_t and get x0_out = 0.  x0_out is required and receives x0' (self-conditioning and the multistep history see
 * the corrected prediction).  There is no initial state (x_t == NULL is DIQT_E_ALIGN): the plain entries make it.  x_next may alias
 * x_t and x0_out may alias x0_prev: a thread reads and writes only the voxels of cells its block owns, each read before it is written;
 * meas_up may alias neither output.  No atomics, no waiting across blocks: bit-reproducible, and with stride = P and unit taps the
 * chain is diqt_cell_project followed by the per-window step, bit for bit.  D % fz, H % fy or W % fx != 0, or a lattice that does
 * not match: DIQT_E_SHAPE; form outside {0, 1, 2} or clamp_mode outside {0, 1}: DIQT_E_UNSUPPORTED.                                */
int diqt_volume_joint_consistent_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                      const float* meas_up, float* x_next, float* x0_out, int form, int N, int D, int H, int W, int P,
                                      int stride, int G0, int G1, int G2, int fz, int fy, int fx, float weight, float kx, float k0,
                                      float kp, float kn, float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw,
                                      unsigned sample, void* stream);
/* The same three entries for a measurement with a SLICE PROFILE: per cell y = sum u[q] x[q], u >= 0 and sum u = 1, q the voxel's
 * lexicographic (z, y, x) index inside its cell (a voxel in a slice gap has u = 0).  The cells stay disjoint, so A A^T = |u|^2 I and
 * A+ = A^T / |u|^2.  `table` is device fp32 [2][n]: u[0 .. n), then the gain g[q] = u[q] / sum u^2 (the uniform profile: u = 1 / n and
 * g = 1).  meas_up is replicated as above.  The projection, in fp32 with no contraction, ONE definition for the three entries:
 *     s = 0;  s = fmaf(u[q], a[q], s) over the cell's voxels in lexicographic order;  m = s           (no division)
 *     t = w * g[q] (one rounded product);  a'[v] = fmaf(t, meas_up[v] - m, a[v])
 * (w = 1: u . a' = y to fp32 rounding; a gap voxel is never moved).  The error codes are those of the uniform entries, a null table
 * being a null pointer; the table's values are the caller's (ops.cell_profile makes them on the host).
 *
 * diqt_cell_wmean: out [D / fz][H / fy][W / fx] = m of x [D][H][W] -- A itself.  out may not alias x.                              */
int diqt_cell_wmean(const float* x, const float* table, float* out, int D, int H, int W, int fz, int fy, int fx, void* stream);
/* diqt_cell_project with that arithmetic: the same cubes, clamp modes and aliasing (out may alias x0; meas_up and table may not
 * alias out).                                                                                                                       */
int diqt_cell_project_profile(const float* x0, const float* meas_up, const float* table, float* out, size_t cubes, int P, int fz, int fy,
                              int fx, float weight, float lo, float hi, int clamp_mode, void* stream);
/* diqt_volume_joint_consistent_step with that arithmetic between the fuse and the update: the forms, the window walk, the normals,
 * the aliasing rules and the error codes are its own, and a cell is corrected only when ALL n of its voxels are covered, whatever
 * their weights.  The table rides in LDS (2n floats more than the uniform entry).  With stride = P and unit taps the chain is
 * diqt_cell_project_profile followed by the per-window step, bit for bit.                                                          */
int diqt_volume_joint_consistent_profile_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                              const float* meas_up, const float* table, float* x_next, float* x0_out, int form, int N,
                                              int D, int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx,
                                              float weight, float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                              unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* NOISE-AWARE consistency (DDNM+, Wang et al. 2023, section 3.3) for a measurement with noise of a known standard deviation: a step
 * projects with its own weight and takes its fresh normals reduced in the range of A,
 *     eps' = eps - shrink g (u . eps)   per cell,   0 < shrink <= 1,
 * which is the projection above applied to the normals with a zero measurement, in the same fp32 arithmetic and the same order:
 *     uniform (table == NULL): m = cell mean of eps;  eps'[v] = fmaf(shrink, 0 - m, eps[v])
 *     profile:                 m = u . eps;  t = shrink * g[q];  eps'[v] = fmaf(t, 0 - m, eps[v])
 * The normals are never clamped.  The weights and shrinks of a chain come from the host (ops.consistency_noise_schedule).
 *
 * diqt_cell_project_noise: diqt_cell_project (table == NULL) or diqt_cell_project_profile on x0 -- the same clamp modes -- and the
 * shaping of `noise`, a tensor of x0's shape, in ONE launch: bit for bit the projection entry on (x0, meas_up, weight, clamp) and the
 * same entry on (noise, zeros, shrink, no clamp).  out_x0 may alias x0 and out_noise may alias noise; nothing else may alias an
 * output.  0 < weight <= 1 and 0 < shrink <= 1, else DIQT_E_UNSUPPORTED.                                                            */
int diqt_cell_project_noise(const float* x0, const float* meas_up, const float* noise, const float* table, float* out_x0,
                            float* out_noise, size_t cubes, int P, int fz, int fy, int fx, float weight, float shrink, float lo, float hi,
                            int clamp_mode, void* stream);
/* diqt_volume_joint_consistent_profile_step with a nullable table (NULL: the uniform operator of diqt_volume_joint_consistent_step)
 * and the step's normal shaped before it enters the update.  Forms 0 and 2 only: form 1, kn == 0 or a shrink outside (0, 1] is
 * DIQT_E_UNSUPPORTED.  The normal of a voxel is the one the plain entries draw (same key, same draw number, one Philox call); it is
 * kept in a third LDS array of the box (at most 16 KiB more) and a cell whose voxels are ALL covered takes eps' above, its sum formed
 * in the order of the x0 sum.  A cell with an uncovered voxel keeps its plain x0 and its plain normals.  Aliasing, geometry and the
 * other error codes are the consistent entries'.  With stride = P and unit taps the chain is diqt_cell_project_noise followed by the
 * per-window step, bit for bit.                                                                                                    */
int diqt_volume_joint_consistent_noise_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                            const float* meas_up, const float* table, float* x_next, float* x0_out, int form, int N,
                                            int D, int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx,
                                            float weight, float shrink, float kx, float k0, float kp, float kn, float lo, float hi,
                                            int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* Data consistency for a TILE-LOCAL LINEAR OPERATOR (ops.tile_operator): the volume splits into disjoint tiles of (fz, fy, fx) voxels,
 * n = fz fy fx in 2 .. 64, and every tile is measured by the same m x n matrix A, m >= 1 rows of any rank (orthogonal thick-slice
 * stacks, a block-DCT low-pass, a partial-volume model).  x0' = x0 + w A+(y - A x0) = x0 + w (t - P x0) with t = A+ y on the high-res
 * grid and P = A+ A, the n x n orthogonal projector onto the row space of A.  `table` is device fp32 [n][n] = P, symmetric to the bit
 * (the caller's: ops.tile_operator makes it on the host).  The projection of the values a of one tile, in fp32 with no contraction, ONE
 * definition for the two projecting entries; q, r = lexicographic (z, y, x) indices inside the tile:
 *     s = 0;  s = fmaf(P[r][q], a[r], s) for r = 0 .. n - 1;  a'[q] = fmaf(w, t[q] - s, a[q])
 * The error codes are those of the cell entries (null pointer, n outside 2 .. 64 or a weight outside (0, 1], a cell that does not
 * divide the volume, m < 1 is DIQT_E_SHAPE).
 *
 * diqt_tile_measure: out [m][D / fz][H / fy][W / fx] = A applied to every tile of x [D][H][W], A device fp32 [m][n]:
 * s = fmaf(A[row][r], x[r], s) in the order of r.  diqt_tile_backproject: out [D][H][W] = t = A+ y, y as diqt_tile_measure writes it,
 * Ap device fp32 [n][m]: s = fmaf(Ap[q][row], y[row], s) in row order.  Neither output may alias an input.                          */
int diqt_tile_measure(const float* x, const float* A, float* out, int m, int D, int H, int W, int fz, int fy, int fx, void* stream);
int diqt_tile_backproject(const float* y, const float* Ap, float* out, int m, int D, int H, int W, int fz, int fy, int fx, void* stream);
/* diqt_cell_project's cubes, clamp modes and aliasing (out may alias x0; target and table may not alias out) with that arithmetic:
 * a = clamp(x0), then the projection onto `target` = t.  A block stages whole tiles in LDS (at most 16 KiB of values and 16 KiB of
 * table) and every voxel has a thread.                                                                                              */
int diqt_tile_project(const float* x0, const float* target, const float* table, float* out, size_t cubes, int P, int fz, int fy, int fx,
                      float weight, float lo, float hi, int clamp_mode, void* stream);
/* diqt_volume_joint_consistent_step with that arithmetic between the fuse and the update, meas_up = t: the forms, the window walk, the
 * normals, the aliasing rules and the error codes are its own, and a tile is corrected only when ALL n of its voxels are covered.  The
 * table rides in LDS behind the box (n^2 floats, at most 16 KiB; a plan above 64 KiB is DIQT_E_SHAPE).  With stride = P and unit taps
 * the chain is diqt_tile_project followed by the per-window step, bit for bit.                                                      */
int diqt_volume_joint_consistent_tile_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                           const float* meas_up, const float* table, float* x_next, float* x0_out, int form, int N, int D,
                                           int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx, float weight,
                                           float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                           unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* NOISE-AWARE consistency for a tile operator (DDNM+ with one weight per singular direction; ops.tile_noise_operator,
 * ops.tile_noise_tables): the rows of A carry noise of their own deviations, so a step moves every right singular direction of the
 * whitened operator by its own lambda and reduces the step's normals there by its own shrink.  `tables` is device fp32 [2][n][n] =
 * M, G of ONE step, M = V diag(lambda) V^T and G = V diag(shrink) V^T, each symmetric to the bit (the caller's).  The arithmetic on the
 * values a, the back-projected measurement t and the normals eps of one tile, fp32 with no contraction, ONE definition for both entries:
 *     d[r] = t[r] - a[r];  s = 0;  s = fmaf(M[r][q], d[r], s) for r = 0 .. n - 1;  a'[q] = a[q] + s;
 *     g = 0;  g = fmaf(G[r][q], eps[r], g) for r = 0 .. n - 1;  eps'[q] = eps[q] - g.     The normals are never clamped.
 * diqt_tile_project_noise is the per-window step (imagen_pytorch3D.py, Imagen.p_sample_loop; elucidated_imagen.py,
 * ElucidatedImagen._dpmpp2m_sample): diqt_tile_project's cubes and clamp modes, a = clamp(x0), `noise` a tensor of x0's shape.  A
 * block reads its voxels before its barrier and writes them after it: out may alias x0 and out_noise may alias noise; nothing else may
 * alias an output.  LDS: three box arrays and 2 n^2 floats; a plan above 64 KiB is DIQT_E_SHAPE.  Null pointer DIQT_E_ALIGN, a cell
 * with n outside 2 .. 64 or a clamp_mode outside 0 .. 2 DIQT_E_UNSUPPORTED, a cell that does not divide P DIQT_E_SHAPE.              */
int diqt_tile_project_noise(const float* x0, const float* target, const float* noise, const float* tables, float* out, float* out_noise,
                            size_t cubes, int P, int fz, int fy, int fx, float lo, float hi, int clamp_mode, void* stream);
/* diqt_volume_joint_consistent_tile_step with that arithmetic between the fuse and the update (inference.py, VolumeInference._chain):
 * a = the fused x0, meas_up = t, eps = the step's Philox normals (key, draw and sample as the plain launch: the same normals), drawn
 * in pass 1.  A tile is corrected and its normals shaped only when ALL n of its voxels are covered; otherwise it keeps its plain x0 and
 * its plain normals.  Forms 0 and 2 with kn != 0 only (DIQT_E_UNSUPPORTED otherwise); window walk, aliasing pairs, uncovered voxels,
 * the x0_out requirement and the other error codes are diqt_volume_joint_consistent_tile_step's.  LDS: the taps, four box arrays and
 * 2 n^2 floats (n = 64: 32 KiB of tables); a plan above 64 KiB -- n = 64 with a box of 2048 voxels or more -- is DIQT_E_SHAPE.       */
int diqt_volume_joint_consistent_tile_noise_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                 const float* x0_prev, const float* meas_up, const float* tables, float* x_next,
                                                 float* x0_out, int form, int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                                 int G2, int fz, int fy, int fx, float kx, float k0, float kp, float kn, float lo, float hi,
                                                 int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* Data consistency for OVERLAPPING SLICE PROFILES (the slab operator; ops.slab_profile).  Slice s of the in-plane cell (cy, cx)
 * measures  y_s = sum_{i < L} u_z[i] (u_yx . x[s fz - r + i, cell]),  L = fz + 2r with reach 1 <= r and 2r <= fz, u_z and u_yx >= 0
 * with sum 1: a slice overlaps its two neighbours only and a voxel lies under at most two slices.  A row is ACTIVE when its whole
 * support lies inside the domain (the cube of the per-window entry, the volume of the joint entries) and is covered; the first and
 * the last slice of a domain never are.  The projection is DDNM on the active rows, x0' = x0 + w A^T (A A^T)^-1 (y - A x0), and
 * A A^T = q G with q = sum u_yx^2 and G Toeplitz tridiagonal (d = sum u_z^2, e = sum_{i < 2r} u_z[i] u_z[i + fz]) on every maximal run
 * of consecutive active rows of a column.  `table` is device fp32, flat (the caller's; ops.slab_profile makes it on the host):
 *     u_z [L], u_yx [fy fx], g_yx = u_yx / q [fy fx], e, m [jmax], ip [jmax]
 * with the pivots pi_0 = d, pi_j = d - e^2 / pi_{j-1} stored as m_j = e / pi_{j-1} (m_0 = 0) and ip_j = 1 / pi_j: no kernel divides.
 * The arithmetic, fp32 with no contraction, ONE definition for all entries:
 *     pm[z] = 0;  pm = fmaf(u_yx[q], a[q], pm) over the fy fx voxels of the plane in (y, x) order
 *     acc = 0;  acc = fmaf(u_z[i], pm[s fz - r + i], acc) over ascending i;  rho_s = y_s - acc, y_s read at voxel (s fz, cy fy, cx fx)
 *     of the replicated measurement
 *     ascending s:   zeta_s = rho_s at run position j = 0, else fmaf(-m_j, zeta_{s-1}, rho_s); a run restarts at j = 0
 *     descending s:  c_s = fmaf(-e, c_{s+1}, zeta_s) * ip_j, c_{s+1} = 0 at the end of a run; inactive rows have c = 0
 *     voxel at depth z = k fz + o:  t = 0;  t = fmaf(u_z[.], c_s, t) over the active ones of s = k - 1 (o < r), k, k + 1 (o >= fz - r)
 *     inside [0, S), ascending;  a' = fmaf(w * g_yx[q], t, a), w * g_yx one rounded product; a voxel under no active row keeps its bits.
 * Error codes: a null pointer DIQT_E_ALIGN; a cell with n outside 2 .. 64, a reach outside the rule, jmax < 1, a weight outside
 * (0, 1] or a clamp mode the entry does not have DIQT_E_UNSUPPORTED; a cell that does not divide the shape, jmax below the number of
 * slices of the domain, an LDS plan above 64 KiB or a workspace that is too small DIQT_E_SHAPE.
 *
 * diqt_slab_measure: out [D / fz][H / fy][W / fx] = A x for x [D][H][W]; a row that leaves the volume takes the truncated sum
 * (outside counts as 0).  out may not alias x.                                                                                      */
int diqt_slab_measure(const float* x, const float* table, float* out, int D, int H, int W, int fz, int fy, int fx, int r, int jmax,
                      void* stream);
/* The per-window step, diqt_cell_project_profile's contract: `cubes` cubes of edge P, a = clamp(x0) with the clamp modes 0 / 1 / 2 of
 * diqt_cell_project, then the projection; out may alias x0 (one thread owns one column (cube, cy, cx) and reads all of it before it
 * writes), meas_up and table may not alias out.  The column's zeta / c live in LDS, P / fz floats per thread of a 256-thread block. */
int diqt_slab_project(const float* x0, const float* meas_up, const float* table, float* out, size_t cubes, int P, int fz, int fy, int fx,
                      int r, int jmax, float weight, float lo, float hi, int clamp_mode, void* stream);
/* The joint path needs a solve along the whole depth of the volume, so a step is THREE launches where the tile-local operators take
 * one.  diqt_volume_joint_slab_coeffs is two of them: per (z, cy, cx) the fy fx voxels are fused as in diqt_volume_joint_step (the
 * same walk and step clamp) into pm and a covered flag; then per column (cy, cx) the rows, the residuals and the two sweeps, c into
 * coef [D / fz][H / fy][W / fx].  `workspace` is device fp32 of at least (2 D + D / fz) (H / fy) (W / fx) floats (pm, the flags, the
 * run positions); the step entry reads the run positions from it, so it must be left alone between the two calls.  meas_up is
 * [D][H][W] in state space.  Nothing here may alias anything else.                                                                 */
int diqt_volume_joint_slab_coeffs(const float* y, const int* slot, const float* taps, const float* meas_up, const float* table,
                                  float* workspace, size_t workspace_floats, float* coef, int N, int D, int H, int W, int P, int stride,
                                  int G0, int G1, int G2, int fz, int fy, int fx, int r, int jmax, float lo, float hi, int clamp_mode,
                                  void* stream);
/* The three update forms of diqt_volume_joint_consistent_step with the correction of a voxel between the fuse and the update, coef
 * and workspace as the call above left them for the same y.  A covered voxel under no active row takes the update with its plain x0;
 * an uncovered voxel keeps x_t and gets x0_out = 0.  Normals and draw numbering are diqt_volume_joint_step's.  x_next may alias x_t
 * and x0_out may alias x0_prev (a thread reads its own voxel of each, then writes it).  No atomics, no waiting across blocks:
 * bit-reproducible, and with the volume equal to one window and unit taps the chain is diqt_slab_project followed by the per-window
 * step, bit for bit.                                                                                                                */
int diqt_volume_joint_consistent_slab_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                           const float* table, const float* coef, const float* workspace, size_t workspace_floats,
                                           float* x_next, float* x0_out, int form, int N, int D, int H, int W, int P, int stride, int G0,
                                           int G1, int G2, int fz, int fy, int fx, int r, int jmax, float weight, float kx, float k0,
                                           float kp, float kn, float lo, float hi, int clamp_mode, unsigned long long seed,
                                           unsigned draw, unsigned sample, void* stream);
/* Data consistency for a K-SPACE BAND LIMIT (the band operator; ops.band_table).  The measurement is the central, box-shaped part of
 * the k-space of a PERIODIC domain (the cube of the per-window entry, the volume of the others), sampled on the low-res grid: on an
 * axis of N voxels with factor f and n = N / f it keeps the frequencies |k| <= kappa = floor((n - 1) / 2) with weights h_k (h_0 = 1,
 * a zero drops a frequency; on an even n the unpaired Nyquist bin is not measured), at an offset of delta voxels.  A, A+ and P = A+ A
 * are Kronecker products over the axes of real circulants, with K the kept k >= 1 and m an index mod N:
 *     P[i][j]  = d[(i - j) mod N],    d[m] = (1 + 2 sum_K cos(2 pi k m / N)) / N                       symmetric to the bit
 *     A[s][j]  = a[(s f - j) mod N],  a[m] = (1 + 2 sum_K h_k cos(2 pi k (m + delta) / N)) / N         rows sum to 1
 *     A+[j][s] = g[(s f - j) mod N],  g[m] = (1 + 2 sum_K (1 / h_k) cos(2 pi k (m + delta) / N)) / n
 * `table` is device fp32, flat (the caller's; ops.band_table makes it on the host in float64, every entry rounded once): for z, then
 * y, then x the tables d [N], a [N], g [N] of the axis.  `active` is a mask of the axes that have a pass (1 = z, 2 = y, 4 = x, not
 * empty): an axis with f = 1 and the full band is the identity and stays out of it -- its pass is skipped, its bits stay; an axis
 * outside the mask must have f = 1.  The arithmetic, fp32 with no contraction, ONE definition for every pass of every entry:
 *     out[i] = acc after  acc = 0;  acc = fmaf(T[idx(i, j)], v[j], acc)  over ASCENDING j along the axis,
 *     idx = (i - j) mod N with T = d,  (i f - j) mod N with T = a,  (j f - i) mod N with T = g (j runs over the n rows);
 * P and A take their passes in the order z, y, x, A+ in the order x, y, z.  The periodic wrap is part of the model.
 * Error codes: a null pointer or an aliasing the entry does not allow DIQT_E_ALIGN; a cell with fz fy fx outside 2 .. 64, an empty
 * mask, an inactive axis with f > 1, a weight outside (0, 1], a form or a clamp mode the entry does not have DIQT_E_UNSUPPORTED; an
 * axis above 512 voxels, a factor that does not divide its axis, an LDS plan above 64 KiB or a workspace that is too small
 * DIQT_E_SHAPE.  One pass plans (2 N + 128 + 64 * 65) floats of LDS.
 *
 * diqt_band_measure: out [D / fz][H / fy][W / fx] = A x for x [D][H][W].  diqt_band_backproject: out [D][H][W] = A+ y.  Each is one
 * launch per active axis; with more than one, `workspace` (device fp32) must hold twice the largest intermediate array -- 2 D H W
 * floats always suffice.  Nothing may alias anything else.  Once per volume.                                                          */
int diqt_band_measure(const float* x, const float* table, float* out, float* workspace, size_t workspace_floats, int D, int H, int W,
                      int fz, int fy, int fx, int active, void* stream);
int diqt_band_backproject(const float* y, const float* table, float* out, float* workspace, size_t workspace_floats, int D, int H, int W,
                          int fz, int fy, int fx, int active, void* stream);
/* The per-window step, diqt_cell_project_profile's contract: `cubes` cubes of edge P, a = clamp(x0) with the clamp modes 0 / 1 / 2 of
 * diqt_cell_project, then the tile operator's projection onto the target t = A+ y (diqt_band_backproject of the cube's measurement):
 *     r = t - a (formed in the loader of the first pass);  c = P r;  out = fmaf(w, c, a) (formed in the storer of the last pass).
 * `workspace` holds two cube batches, 2 cubes P^3 floats, and every pass but the last writes there, so out may alias x0; target, table
 * and the workspace may not alias out or x0.  With one active axis the only pass stores c and a fourth, elementwise launch forms
 * out.  One launch per active axis (plus that one).                                                                                  */
int diqt_band_project(const float* x0, const float* target, const float* table, float* workspace, float* out, size_t cubes, int P, int fz,
                      int fy, int fx, size_t workspace_floats, int active, float weight, float lo, float hi, int clamp_mode, void* stream);
/* out [D][H][W] = P x: the projector's passes over a volume, through out itself and `workspace` (D H W floats); x, out and the
 * workspace are three different volumes.                                                                                             */
int diqt_band_apply(const float* x, const float* table, float* out, float* workspace, size_t workspace_floats, int D, int H, int W,
                    int active, void* stream);
/* The joint path: the projector crosses every window border, so a step is three calls -- diqt_volume_joint_band_residual,
 * diqt_band_apply on r, diqt_volume_joint_consistent_band_step -- and up to five launches.  The first fuses every voxel as
 * diqt_volume_joint_step does (the same walk and step clamp) and writes three [D][H][W] volumes: a_out the fused clamped prediction
 * (0 where no kept window covers), covered_out 1 / 0, and r_out = target - a, or 0 where nothing covers: there the measurement is
 * believed, so the projection is exact (A x0' = y at w = 1) only on a fully covered volume.  target is t = A+ y in state space.      */
int diqt_volume_joint_band_residual(const float* y, const int* slot, const float* taps, const float* target, float* a_out,
                                    float* covered_out, float* r_out, int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                    int G2, float lo, float hi, int clamp_mode, void* stream);
/* The three update forms of diqt_volume_joint_consistent_step on x0' = fmaf(w, c, a) per covered voxel, with a and covered as the
 * residual call left them and c = P r from diqt_band_apply.  The windows are not walked again: y, slot, taps, the lattice and the
 * clamp are not looked at.  An uncovered voxel keeps x_t and gets x0_out = 0.  Normals and draw numbering are
 * diqt_volume_joint_step's.  x_next may alias x_t and x0_out may alias x0_prev (a thread reads its own voxel of each, then writes
 * it).  No atomics, no waiting across blocks: bit-reproducible, and with the volume equal to one window and unit taps the chain is
 * diqt_band_project followed by the per-window step, bit for bit.                                                                    */
int diqt_volume_joint_consistent_band_step(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                           const float* a, const float* covered, const float* c, float* x_next, float* x0_out, int form,
                                           int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx,
                                           float weight, float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                           unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* The stochastic Heun sampler of the EDM family (Karras et al. 2022; elucidated_imagen.py:382-532) on the joint state: a churn, a
 * predictor and a corrector per step, two U-Net evaluations.  The state is three [D][H][W] volumes, all updated in place (every thread
 * reads only its own voxel of each, then writes it): xh = images_hat, xn = images_next, x0 = the fused prediction.  Window walk,
 * clamp, lattice check, launch geometry and the normals n(draw) are diqt_volume_joint_step's.  `phase`, uniform over the launch:
 *   0  xh = fmaf(kc, n(draw + 1), a * n(draw)) with the product rounded first (a = sigma0: the initial image as the sampler stores
 *      it, then the churn of step 0; no second Philox call when kc == 0).  Every voxel; y, slot, taps, xn, x0, N, P, stride, G*, b, c,
 *      d and the clamp are ignored.
 *   1  after the stage-0 evaluations (y = the windows' predictions at sigma_hat): covered voxel x0 = num / den,
 *      xn = fmaf(b, x0, a * xh), the Euler predictor with (a, b) = (1 + r, -r); uncovered voxel xn = xh, x0 = 0.  c, d, kc, seed,
 *      draw and sample are ignored.
 *   2  after the stage-1 evaluations (y = the predictions at sigma_next): covered voxel x0b = num / den,
 *      t = fmaf(c, xn, fmaf(b, x0, a * xh)), x = fmaf(d, x0b, t), the corrector with (a, b, c, d) = (1 + r/2, -r/2, r2, -r2); then the
 *      next step's churn xh = fmaf(kc, n(draw), x) (xh = x, no Philox call, when kc == 0) and x0 = x0b.  Uncovered voxel: xh is left
 *      as it is, x0 = 0.
 * These are the roundings of the diqt_axpby3 sequence of the per-window sampler, so with stride = P and unit taps the chain is that
 * sampler's bit for bit.  Null pointers: DIQT_E_ALIGN; a lattice that does not match: DIQT_E_SHAPE; phase outside {0, 1, 2} or
 * clamp_mode outside {0, 1}: DIQT_E_UNSUPPORTED; phase 0 with draw == 2^32 - 1: DIQT_E_SHAPE.                                      */
int diqt_volume_joint_heun(const float* y, const int* slot, const float* taps, float* xh, float* xn, float* x0, int phase, int N, int D,
                           int H, int W, int P, int stride, int G0, int G1, int G2, float a, float b, float c, float d, float kc,
                           float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream);
/* Phases 1 and 2 of diqt_volume_joint_heun with the data-consistency projection between the fuse and the update (DDNM on both
 * predictions of a Heun step, or on the predictor's alone when only phase 1 goes through here): in every cell whose voxels are ALL
 * covered the fused prediction becomes x0' = x0 + w A+(y - A x0), and the phase's update reads x0' where the plain launch reads the
 * fused x0; a cell with an uncovered voxel is left alone, and an uncovered voxel is treated as there (phase 1: xn = xh, x0 = 0; phase
 * 2: xh untouched, x0 = 0).  `mode` chooses the projection, each the ONE definition of its per-window entry: 0 the cell mean
 * (diqt_cell_project; `table` is not looked at), 1 a slice profile (diqt_cell_project_profile; `table` device fp32 [2][n]), 2 a
 * tile operator (diqt_tile_project; `table` device fp32 [n][n] = P and meas_up = t).  `meas_up` [D][H][W] is in state space; the cell
 * (fz, fy, fx), n = fz fy fx in 2 .. 64, must divide D, H and W; weight in (0, 1].  The geometry is diqt_volume_joint_consistent_step's:
 * a block owns a box of whole cells, fuses it into LDS and revisits it after ONE barrier, so xh, xn and x0 are updated in place with
 * no atomics and no waiting across blocks -- bit-reproducible.  There is no phase 0: the initial state is diqt_volume_joint_heun's.
 * Coefficients, kc, the clamp, the normals and their numbering are that entry's.  With stride = P and unit taps the chain is the
 * per-window Heun loop with the mode's projection launch after an evaluation, bit for bit.  Null pointers (table only for mode 0):
 * DIQT_E_ALIGN; phase outside {1, 2}, mode outside {0, 1, 2}, n outside 2 .. 64, a weight outside (0, 1] or clamp_mode outside
 * {0, 1}: DIQT_E_UNSUPPORTED; a cell that does not divide the volume, a lattice that does not match or a plan above 64 KiB of LDS
 * (the taps, two box arrays and the table): DIQT_E_SHAPE.                                                                          */
int diqt_volume_joint_consistent_heun(const float* y, const int* slot, const float* taps, float* xh, float* xn, float* x0,
                                      const float* meas_up, const float* table, int phase, int mode, int N, int D, int H, int W, int P,
                                      int stride, int G0, int G1, int G2, int fz, int fy, int fx, float weight, float a, float b, float c,
                                      float d, float kc, float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw,
                                      unsigned sample, void* stream);
/* One pass boundary of the inpainting (RePaint) loop around that sampler, per window batch (elucidated_imagen.py:479-486 and 520-523:
 * `images = images + (sigma - sigma_next) * repaint_noise`, then `images_hat = images + added_noise` with the known image under the
 * mask) -- the re-noise that ends pass r, the paste and the churn that begins the next pass in ONE launch, in place of two diqt_axpby3
 * and one selection with two temporaries.  x / renoise / known / eps / out are [B][per_batch], mask one byte per element (non-zero:
 * known), kr / kc DEVICE [B]:
 *     t = renoise ? fmaf(kr, renoise, x) : x;  u = mask ? known : t;  out = fmaf(kc, eps, u)
 * -- the roundings of diqt_axpby3(x, renoise, 1, kr) and diqt_axpby3(u, eps, 1, kc) with a pure selection between them; the churn
 * product is fused in also when kc == 0, as diqt_axpby3 does it.  renoise == NULL: no re-noise, kr is not read.  out may alias x (every
 * thread reads its own element, then writes it).  Null pointers: DIQT_E_ALIGN; B <= 0, per_batch == 0 or B > 65535: DIQT_E_SHAPE.   */
int diqt_edm_inpaint_churn(const float* x, const float* renoise, const float* known, const unsigned char* mask, const float* eps,
                           const float* kr, const float* kc, float* out, int B, size_t per_batch, void* stream);
/* The same loop on the joint state: diqt_volume_joint_heun plus known [D][H][W] (in state space), mask (uint8 [D][H][W]), kr and a
 * second draw index.  The predictor is phase 1 of diqt_volume_joint_heun, unchanged.  `phase` here:
 *   0  xh = sel(m, known, a * n(draw)) + kc * n(draw + 1): the initial image, the paste, the churn of step 0.  Every voxel; the
 *      window arguments, xn, x0, b, c, d, kr, draw_r and the clamp are ignored.
 *   2  the corrector of diqt_volume_joint_heun's phase 2 up to x; where kr != 0, x = fmaf(kr, n(draw_r), x), the re-noise that ends a
 *      pass that is not the last of its step; then xh = sel(m, known, x) + kc * n(draw) and x0 = x0b.  Uncovered voxel: xh is left
 *      as it is, x0 = 0.
 *   3  xh = sel(m, known, xn) + kc * n(draw): the further passes of the step that ends at sigma 0, which has no corrector.  Every
 *      voxel, no window walk; the window arguments, x0, a .. d, kr, draw_r and the clamp are ignored.
 * sel and the two updates are diqt_edm_inpaint_churn's; with kc == 0 the churn is the selection alone and no normal is computed (the
 * per-window pass differs from that in the sign of a zero at most).  Null pointers: DIQT_E_ALIGN; a lattice that does not match
 * (phase 2): DIQT_E_SHAPE; a phase outside {0, 2, 3} or clamp_mode outside {0, 1}: DIQT_E_UNSUPPORTED; phase 0 with draw == 2^32 - 1:
 * DIQT_E_SHAPE.                                                                                                                   */
int diqt_volume_joint_heun_inpaint(const float* y, const int* slot, const float* taps, float* xh, const float* xn, float* x0,
                                   const float* known, const unsigned char* mask, int phase, int N, int D, int H, int W, int P,
                                   int stride, int G0, int G1, int G2, float a, float b, float c, float d, float kr, float kc, float lo,
                                   float hi, int clamp_mode, unsigned long long seed, unsigned draw, unsigned draw_r, unsigned sample,
                                   void* stream);
/* One pass boundary of the inpainting (RePaint) loop around the ancestral sampler of the DDPM family, per window batch
 * (imagen_pytorch3D.py:2139-2146, `renoised_img = noise_scheduler.q_sample_from_to(img, times_next, times)`, then :2119-2123 of the
 * next pass, `noised_inpaint_images = noise_scheduler.q_sample(inpaint_images, t = times)` under the mask) -- the re-noise that ends
 * pass r and the paste that begins the next pass in ONE launch, in place of diqt_axpby3, diqt_q_sample and diqt_mask_blend with two
 * temporaries and a float mask.  x / renoise / known / qnoise / out are [B][per_batch], mask one byte per element (non-zero: known),
 * kr0 / kr1 / al / sg DEVICE [B]:
 *     t = renoise ? fmaf(kr1, renoise, kr0 * x) : x;  out = mask ? fmaf(sg, qnoise, al * known) : t
 * -- the roundings of diqt_axpby3(x, renoise, kr0, kr1) and of diqt_q_sample(known, qnoise, al, sg), which is diqt_axpby3, with
 * diqt_mask_blend's pure selection behind them.  renoise == NULL: no re-noise, kr0 and kr1 are not read (the first paste of a chain,
 * the first pass of a step, every pass of the step that ends at t = 0).  out may alias x (every thread reads its own element, then
 * writes it).  Error codes and limits are diqt_edm_inpaint_churn's.                                                                */
int diqt_ddpm_inpaint_paste(const float* x, const float* renoise, const float* known, const unsigned char* mask, const float* qnoise,
                            const float* kr0, const float* kr1, const float* al, const float* sg, float* out, int B, size_t per_batch,
                            void* stream);
/* The same loop on the joint state: the first-order step of diqt_volume_joint_step, in place on x, plus known [D][H][W] (in state
 * space), mask (uint8 [D][H][W]), the pass boundary's coefficients and three draw indices.  `phase`:
 *   0  x = m ? fmaf(sg, n(draw_q), al * known) : n(draw): the initial image (:2080) under the first paste (:2119-2123).  Every voxel;
 *      the window arguments, x0_out, flags, kx .. kr1, draw_r and the clamp are ignored.
 *   1  x0 = sum(w c(y)) / sum(w) and u = kx x + k0 x0 + kn n(draw) exactly as diqt_volume_joint_step forms them (the product added
 *      also when it is 0, no normal computed when kn == 0); `flags` bit 0: u = fmaf(kr1, n(draw_r), kr0 * u), the re-noise that ends a
 *      pass which is not the last of its step (:2139-2146); bit 1: x = m ? fmaf(sg, n(draw_q), al * known) : u, the paste that begins
 *      the next pass, (al, sg) being THAT pass's step's; else x = u.  x0_out (may be NULL) = x0.  Uncovered voxel: x is left as it
 *      is, x0_out = 0.
 * The two updates are diqt_ddpm_inpaint_paste's, so at stride = patch the chain is the per-window loop bit for bit.  A thread computes
 * only the normals whose result it stores: a masked voxel with a paste following n(draw_q) alone.  known / mask / x null, or a window
 * pointer in phase 1: DIQT_E_ALIGN; a lattice that does not match (phase 1): DIQT_E_SHAPE; a phase outside {0, 1}, flags outside
 * 0 .. 3 or clamp_mode outside {0, 1}: DIQT_E_UNSUPPORTED.                                                                        */
int diqt_volume_joint_step_inpaint(const float* y, const int* slot, const float* taps, float* x, float* x0_out, const float* known,
                                   const unsigned char* mask, int phase, int flags, int N, int D, int H, int W, int P, int stride,
                                   int G0, int G1, int G2, float kx, float k0, float kn, float kr0, float kr1, float al, float sg,
                                   float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw, unsigned draw_r,
                                   unsigned draw_q, unsigned sample, void* stream);
/* The end of sample s (0-based) of S joint chains: per voxel r = min_val where vol (RAW, may be NULL) has (vol - mean) / std ==
 * min_val (diqt_background_reset's expression), else x (the finished state) where a kept window (slot >= 0) covers the voxel, else
 * `fill`; then diqt_volume_blend's Welford update in sample order, delta = r - m; m += delta / (s + 1); m2 = fma(delta, r - m, m2)
 * on (mean_io, m2_io), which sample 0 initialises (they are not read then).  With s == S - 1 and out_std non-NULL, out_std =
 * sqrt(m2 / (S - 1)).  m2_io and out_std must be NULL for S == 1; m2_io may be NULL when no deviation map is wanted.            */
int diqt_volume_joint_finish(const float* x, const int* slot, const float* vol, float* mean_io, float* m2_io, float* out_std, int s,
                             int S, int D, int H, int W, int P, int stride, int G0, int G1, int G2, float mean, float stdv,
                             float min_val, float fill, void* stream);

/* ---- training data path + validation metrics on the device ----------------------------------------------
 * data.py:88-137 supervisedIQT.__getitem__: crop a P^3 patch pair out of HBM-resident [V][D][H][W] low-res / high-res volume
 * stacks at sel[n] = {volume, i0, j0, k0} and normalise it: mode 0 (v - mean) / std, mode 1 2*((v - min)/(max - min) - 0.5)
 * with the patch's own extrema (data.py:82-86).  Outputs are [n][P][P][P].  The workspace is only read in mode 1. */
size_t diqt_patch_pair_crop_workspace_bytes(int n_patches, int P);
int diqt_patch_pair_crop(const float* lr_vols, const float* hr_vols, const int* sel, float* lr_out, float* hr_out, void* workspace,
                         size_t workspace_bytes, int n_patches, int V, int D, int H, int W, int P, int mode, float mean, float stdv,
                         void* stream);
/* out2 = {min, max} of x[0..n).  workspace: 8 KiB. */
int diqt_minmax(const float* x, size_t n, void* workspace_8k, float* out2, void* stream);
/* metrics.py:19-23 PSNR -> torchmetrics 0.9.0 peak_signal_noise_ratio(data_range): out2 = {mse, 10 log10(range^2 / mse)} of
 * the tensors after the optional min-max normalisation stats4 = {pred min, pred max, target min, target max} (device, or NULL). */
int diqt_psnr(const float* pred, const float* target, size_t n, const float* stats4, float data_range, void* workspace_8k,
              float* out2, void* stream);
/* metrics.py:25-31 SSIM -> torchmetrics 0.9.0 StructuralSimilarityIndexMeasure on N volumes [D][H][W] (N = batch * channels):
 * K-tap separable Gaussian (taps: HOST pointer, K odd <= 11), constants (k1 range)^2 / (k2 range)^2, mean of the SSIM map over
 * the windows that survive torchmetrics' reflect-pad + crop (= the windows fully inside the volume).  out[0] = SSIM. */
size_t diqt_ssim3d_workspace_bytes(int N, int D, int H, int W, int K);
int diqt_ssim3d(const float* pred, const float* target, int N, int D, int H, int W, const float* taps, int K, const float* stats4,
                float data_range, float k1, float k2, void* workspace, size_t workspace_bytes, float* out, void* stream);
/* metrics.py:32-34 MSSIM, called on every reconstructed volume by test_all.py:56-62 -> torchmetrics 0.9.0
 * MultiScaleStructuralSimilarityIndexMeasure (normalize=None, data_range=None) on N volumes [D][H][W]: per scale the SSIM and the
 * contrast-sensitivity means of diqt_ssim3d's windows with the data range max(p.max - p.min, t.max - t.min) of THAT scale, then a
 * 2x2x2 average pool; out[0] = prod_s term_s ^ betas[s] (term = cs below the last scale, ssim at it; a negative term gives NaN),
 * followed by {ssim_s, cs_s, range_s} per scale (1 + 3 scales floats).  One tile launch per scale produces the sums, the pooled
 * pair and its min / max; a one-workgroup finaliser reduces them in a fixed order.  No host synchronisation.  taps, betas: HOST
 * pointers; 1 <= scales <= 16.  The workspace query returns 0 when an axis has fewer than K voxels at the last scale. */
size_t diqt_msssim3d_workspace_bytes(int N, int D, int H, int W, int K, int scales);
int diqt_msssim3d(const float* pred, const float* target, int N, int D, int H, int W, const float* taps, int K, const float* betas,
                  int scales, float k1, float k2, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* Gradient accumulation (accelerate's accumulate()/DDP no_sync, trainer.py:300,1118): the per-parameter gradients of one
 * micro-step are added into the flat gradient arena in ONE launch.  table[t] = {src device pointer, dst element offset,
 * element count} (3 x int64, device memory); every tensor gets `blocks_per_tensor` workgroups.                    */
int diqt_multi_accumulate(float* dst, const long long* table, int count, int blocks_per_tensor, void* stream);
/* The same with the table in HOST memory: it travels in the kernel arguments (120 rows per launch), so there is no table upload and the
 * launches can be captured into a hipGraph as they stand (the trainer's captured micro-step).                                   */
int diqt_multi_accumulate_host(float* dst, const long long* host_table, int count, int blocks_per_tensor, void* stream);
int diqt_ema_lerp(float* ema, const float* param, size_t n, float one_minus_decay, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention over flattened volumetric tokens.
 * ---------------------------------------------------------------------------------------------- */
/* softmax over the middle axis of x[outer][n][inner] (inner = 1: row softmax), scaled by `scale`
 * after normalisation (LinearAttention imagen_pytorch3D.py:1003-1006; Attention imagen_video.py:511) */
int diqt_softmax_fwd(const float* x, float* y, size_t outer, int n, int inner, float scale, void* stream);
int diqt_softmax_bwd(const float* y, const float* dy, float* dx, size_t outer, int n, int inner, float scale,
                     void* stream);
/* The kernel either of them launches, as a pure shape query: 0 a workgroup per long row (inner 1, n >= 4096, outer <= 1024), 1 a wave
 * per row (inner 1), 2 a workgroup per outer index (forward only: inner divides 1024, n >= 64, outer <= 65535), 3 a thread per column. */
int diqt_softmax_route(size_t outer, int n, int inner, int backward);
/* Multi-query attention probabilities (imagen_video.Attention :490-518): sim[G][n][h][M] holds scores of n queries x h
 * heads against M = n_extra + n_self keys ordered [context..., null, self...]; adds rel[(i-j+n_self-1)][h] (T5-style
 * DynamicPositionBias table, may be NULL) on self keys and null_bias[h] (may be NULL) on the null key (the last extra
 * key), masks self keys j > i when causal, and soft-maxes over M in place layout.  bwd also accumulates drel / dnull
 * (zeroed by the caller; float atomics).  DIQT_E_SHAPE: fwd with causal or rel, bwd with drel, when n_self != n (the table
 * index would leave the table); null_bias / dnull_bias without an extra key.                                     */
int diqt_attn_softmax_fwd(const float* sim, const float* rel, const float* null_bias, float* p,
                          int G, int n, int h, int n_extra, int n_self, int causal, void* stream);
int diqt_attn_softmax_bwd(const float* p, const float* dp, float* dsim, float* drel, float* dnull_bias,
                          int G, int n, int h, int n_extra, int n_self, int causal, void* stream);
/* Same gradients with the relative-bias / null-bias sums reduced in a fixed order through `workspace`
 * (diqt_attn_softmax_bwd_workspace_bytes; 0 = table too large, the call falls back to the atomic kernel). */
size_t diqt_attn_softmax_bwd_workspace_bytes(int G, int n, int h, int n_extra, int n_self);
int diqt_attn_softmax_bwd_ws(const float* p, const float* dp, float* dsim, float* drel, float* dnull_bias,
                             void* workspace, size_t workspace_bytes, int G, int n, int h, int n_extra, int n_self,
                             int causal, void* stream);
/* Fused multi-query attention forward for the sampling path (imagen_video.py:410-525 Attention.forward): q[G][n][h][d],
 * kv[G][n_extra + n_self][2d] (k | v per key row; extra keys first, learned null key last of them), optional relative
 * position table rel[2n-1][h] on the self keys with null_bias[h] on the null key, optional causal mask ->
 * out[G][n][h*d] = softmax(scale q.k + bias) v.  The [G, n*h, keys] score tensor is never materialised.  d = 32 or 64. */
int diqt_mqa_attention_fwd(const float* q, const float* kv, const float* rel, const float* null_bias, float* out, int G,
                           int n, int h, int d, int n_extra, int n_self, int causal, float scale, void* stream);
/* Training path of the same Attention.forward (imagen_video.py:483-520 `sim = einsum(...)`, `sim.softmax`, `einsum(attn, v)` and
 * their autograd backward): the forward additionally writes lse[G][n*h] (row log-sum-exp), and the backward recomputes the
 * probabilities from it instead of reading a stored [G, n*h, keys] tensor:
 *   dq[G][n*h][d], dkv[G][n_extra + n_self][2d] (every row written: the extra rows carry the gradient of the null / context
 *   keys), drel[2 n_self - 1][h] and dnull[h] (required iff rel / null_bias are given).
 * Deterministic (no atomics; bias tables are summed per wave, then in a fixed order).  workspace: ..._bwd_workspace_bytes. */
/* The temporal attentions of the pseudo-3D U-Net -- EinopsToAndFrom('b c f h w', '(b h w) f c', Attention), imagen_video.py:1351-1354,
 * 410-525 -- on the channels-last tensors as they stand: q[B][F][P][h d], kv[B][F][P][2 d] (k | v of frame f at pixel p), out like q.
 * A sequence is (b, p), its tokens the F frames; one extra key / value nullkv[2 d] in front (the learned null row; null_bias[h] is
 * added to its score when rel is given).  Replaces the two mid-axis transposes and the null-row concatenation around
 * diqt_mqa_attention_fwd; same kernel, bit-identical results.                                                                      */
int diqt_mqa_attention_fwd_frames(const float* q, const float* kv, const float* nullkv, const float* rel, const float* null_bias,
                                  float* out, int B, int F, int P, int h, int d, int causal, float scale, void* stream);
/* The whole temporal attention block of the pseudo-3D U-Net as one kernel (sampling path under autocast): per sequence (b, p) of F frames
 *     y = LayerNorm(Attention(LayerNorm(x; norm_g)) W_o; out_g) + x
 * -- Residual(EinopsToAndFrom('b c f h w', '(b h w) f c', Attention(dim, causal, rel_pos_bias))), imagen_video.py:1351-1354, 410-525 --
 * on x[B][F][P][C] fp32 as it stands.  16-bit MFMA operands (fp16, or bf16 when `bf16`), fp32 accumulation, soft-max and LayerNorms;
 * q, k, v, scores and head outputs never leave the CU.  Weights, 16-bit: wq_h[h d][C] = scale * to_q.weight, wkv_h[2 d][C] =
 * to_kv.weight, wo_h[h][C][d] = to_out.weight[c][head d] with the 64 channels of a head in the accumulator order
 * pos(d) = 16 (d >> 4) + 8 ((d >> 2) & 1) + 4 ((d >> 3) & 1) + (d & 3).  null_kv[2][d], rel[2F-1][h] / null_bias[h] (both or neither).
 * round_out: round the to_out product to the operand type before the LayerNorm (what autocast's Linear returns).
 * Shapes: d = 64, h in {4, 8}, F in {32, 64}, C in {64, 128, 256} (diqt_temporal_attention_h_supported).                              */
int diqt_temporal_attention_h_supported(int B, int F, int P, int C, int h, int d);
int diqt_temporal_attention_h(const float* x, const float* norm_g, const void* wq_h, const void* wkv_h, const void* wo_h,
                              const float* out_g, const float* null_kv, const float* rel, const float* null_bias, float* y,
                              int B, int F, int P, int C, int h, int d, int causal, float eps, int bf16, int round_out, void* stream);
int diqt_mqa_attention_fwd_lse(const float* q, const float* kv, const float* rel, const float* null_bias, float* out, float* lse,
                               int G, int n, int h, int d, int n_extra, int n_self, int causal, float scale, void* stream);
size_t diqt_mqa_attention_bwd_workspace_bytes(int G, int n, int h, int d, int n_extra, int n_self, int has_rel);
/* The plan diqt_mqa_attention_bwd launches from, as a pure shape query (no GPU): `field` 0 the path (0 refused, 1 the one-pass
 * short-sequence kernel, 2 the dQ kernel followed by the dK/dV kernel), 1 the error code of a refusal (0 otherwise), 2 the workgroups
 * that write bias-gradient partials, and of the dK/dV launch 3 key tiles per workgroup KW (0: a sequence per wave), 4 sequence per wave,
 * 5 extra keys taken by the VALU, 6 grid.x, 7 floats of the bias table kept in LDS, 8 whether its XCD remap applies, 9 grid.y; 10 the
 * rows of bias-gradient partials the workspace holds.  Refused: dim_head other than 32 / 64, more than 64 heads, G > 65535, a table
 * of more than 1536 entries.  Leaves diqt_last_error alone.                                                                          */
int diqt_mqa_attention_bwd_route(int G, int n, int h, int d, int n_extra, int n_self, int has_rel, int has_null, int field);
int diqt_mqa_attention_bwd(const float* q, const float* kv, const float* rel, const float* null_bias, const float* out,
                           const float* dout, const float* lse, float* dq, float* dkv, float* drel, float* dnull,
                           void* workspace, size_t workspace_bytes, int G, int n, int h, int d, int n_extra, int n_self,
                           int causal, float scale, void* stream);

/* Mixed-precision variant for torch.autocast (the reference's `einsum('b h i d, b j d -> b h i j')` and `einsum(attn, v)` run in
 * fp16 / bf16 there, its soft-max in fp32; imagen_video.py:483-520): q k^T and p v on v_mfma_f32_32x32x16_{f16,bf16} with fp32
 * accumulation and fp32 soft-max statistics; q and out stay fp32 in HBM, `kv_h` is the 16-bit copy of kv (diqt_cast_to_h: every
 * workgroup streams all keys, so the copy halves the dominant traffic); round_out = 1 rounds the result once to the operand type.
 * Otherwise the arguments and layouts of diqt_mqa_attention_fwd.                                      */
int diqt_mqa_attention_fwd_h(const float* q, const void* kv_h, const float* rel, const float* null_bias, float* out, int G, int n,
                             int h, int d, int n_extra, int n_self, int causal, float scale, int bf16, int round_out, void* stream);
/* The one decision of diqt_mqa_attention_fwd_h as a pure shape query: `field` 0 waves per workgroup (4 or 8), 1 query rows per
 * workgroup, 2 whether the relative-bias instantiation runs.                                                                       */
int diqt_mqa_attention_fwd_h_route(int n, int h, int d, int has_rel, int field);
/* y[i] = (fp16 | bf16) x[i]: the 16-bit copy of the K|V rows that diqt_mqa_attention_fwd_h streams (n even).                   */
int diqt_cast_to_h(const float* x, void* y_h, size_t n, int bf16, void* stream);


/* batched fp32 MFMA GEMM: C[g] = alpha * op(A[g]) * op(B[g]) (+ beta*C[g]); row-major, strides in floats */
int diqt_bgemm(const float* A, const float* Bm, float* C, int batch, int M, int N, int K,
               int transA, int transB, long long strideA, long long strideB, long long strideC,
               int lda, int ldb, int ldc, float alpha, float beta, void* stream);
/* Same GEMM with a caller-owned workspace: problems with few output tiles and a long K (dK / dV of the attentions, 1- and
 * 5-row products) are split along K into slabs that a second kernel sums in a fixed order.
 * diqt_bgemm_workspace_bytes() returns 0 when the shape is not split.                                              */
size_t diqt_bgemm_workspace_bytes(int batch, int M, int N, int K);
int diqt_bgemm_ws(const float* A, const float* Bm, float* C, void* workspace, size_t workspace_bytes, int batch, int M, int N,
                  int K, int transA, int transB, long long strideA, long long strideB, long long strideC, int lda, int ldb,
                  int ldc, float alpha, float beta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIQT_H */
