/*
 * risp.h - C ABI of libreconfigisp_hip.so, the MI355X (gfx950) implementation of
 * ReconfigISP's per-image ISP forward path.
 *
 * What this boundary replaces (paths relative to the reference's codes/):
 *   - the absent /DATA/ISP_Kernels plugin that models/modules/tools_origin.py:8-17
 *     imports and calls as  Kernel().run(img, option, params_dict)  (14 call sites,
 *     SURVEY.md section 8b);
 *   - the torch-eager bodies of the in-tree operators (WbQuadratic, GtmManual, the
 *     SRCNN / Path-Restore proxies, the mixed-op combiner, whole2patch/patch2whole).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  Every pointer is DEVICE memory
 *     owned by the caller (PyTorch); the library keeps no reference past the call and
 *     allocates nothing; scratch space is passed in explicitly.
 *   - tensors are contiguous NCHW fp32; colour images are BGR (ch0=B, ch1=G, ch2=R),
 *     Bayer mosaics are 1-channel RGGB; H and W are even.
 *   - `stream` is a hipStream_t (NULL = default stream); launches are asynchronous.
 *   - return value 0 = OK; non-zero = error, text via risp_last_error() (thread local).
 *   - re-entrant: no mutable global state.
 */
#ifndef RISP_H
#define RISP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RISP_VERSION 100

int risp_version(void);
const char *risp_last_error(void);

/* ---------------------------------------------------------------------------
 * Element-wise operators.  `p` is the (N,P) per-image parameter block in [0,1]
 * (what the reference passes as sigmoid(par).repeat(N,1)); gp is (N,P) and is
 * fully written by the call.
 * ------------------------------------------------------------------------- */

/* demosaic.Demosaic().run(img,'nearestneighbor',..) - tools_origin.py:278-284.
 * (N,1,H,W) RGGB -> (N,3,H,W) BGR.  OPSPEC: R,B replicated over the 2x2 quad,
 * G takes the green sample of its own row. */
int risp_demosaic_nearest_fwd(const float *bayer, float *bgr, int N, int H, int W, void *stream);
int risp_demosaic_nearest_bwd(const float *g_bgr, float *g_bayer, int N, int H, int W, void *stream);

/* whitebalance.WhiteBalance().run(img,'manual',{'gain'}) - tools_origin.py:211-221.  p = the gain
 * itself, (N,3) in [0,5] (the wrapper's params * 5, :214); y_c = x_c * gain_c, no clipping. */
int risp_wb_manual_fwd(const float *x, const float *p, float *y, int N, int HW, void *stream);
/* All *_bwd of the element-wise ops: gp is fully written (no pre-zeroing); scratch holds
 * risp_param_grad_scratch_floats(N) floats - one partial row per workgroup, added in index order by a second
 * launch, so parameter gradients are bit-repeatable. */
size_t risp_param_grad_scratch_floats(int N);
int risp_wb_manual_bwd(const float *x, const float *p, const float *gy, float *gx, float *gp,
        float *scratch, int N, int HW, void *stream);

/* gamma.Gamma().run(img,'manual',{'gamma':g}) - tools_origin.py:59-69. P=1.
 * OPSPEC: y = x^g (x >= 1/1024), y = x * (1/1024)^(g-1) below. */
int risp_gamma_fwd(const float *x, const float *p, float *y, int N, int HW, void *stream);
int risp_gamma_bwd(const float *x, const float *p, const float *gy, float *gx, float *gp,
        float *scratch, int N, int HW, void *stream);

/* GtmManual(4).forward - tools_origin.py:414-440. P=3; knots come from p[0,:] only,
 * so gp[0,:] holds the whole-batch gradient and gp[1:,:] = 0. */
int risp_gtm_manual_fwd(const float *x, const float *p, float *y, int N, int HW, void *stream);
int risp_gtm_manual_bwd(const float *x, const float *p, const float *gy, float *gx, float *gp,
        float *scratch, int N, int HW, void *stream);

/* WbQuadratic.forward - tools_origin.py:317-359. P=30, coef[n,ch,j] = 10 p[n,10ch+j] - 5 */
int risp_wb_quadratic_fwd(const float *x, const float *p, float *y, int N, int HW, void *stream);
int risp_wb_quadratic_bwd(const float *x, const float *p, const float *gy, float *gx, float *gp,
        float *scratch, int N, int HW, void *stream);

/* Per-image per-channel statistics of an (N,C,H,W) tensor (NC = N*C planes):
 * stats[plane*4+{0,1,2}] = {min, sum, max}; arg[plane*2+{0,1}] = first (row-major) index of
 * the min / max (may be NULL).  Used by SRCNNRes (srcnn_res_arch.py:36-40) and gray-world.
 * Any HW > 0: planes of HW % 4 == 0 pixels at a 16-byte aligned x through 16-byte loads, others through element loads.
 * scratch: risp_channel_stats_scratch_floats(NC,HW) floats.  Deterministic (no atomics). */
size_t risp_channel_stats_scratch_floats(int NC, int HW);
int risp_channel_stats(const float *x, float *stats, int32_t *arg, float *scratch, int NC, int HW,
                       void *stream);
/* backward of the statistics, in place on gx (NC planes): gx += g_mean[plane]/HW everywhere,
 * gx[argmin] += g_min[plane], gx[argmax] += g_max[plane]; any of the three may be NULL.  Any HW > 0, as the forward:
 * 16-byte accesses when HW % 4 == 0 and gx is 16-byte aligned, element accesses otherwise. */
int risp_stats_bwd(float *gx, const float *g_min, const float *g_mean, const float *g_max,
                   const int32_t *arg, int NC, int HW, void *stream);
/* the same with the three gradients as column ranges of a row-major (N, row_stride) matrix - plane n * C + c reads
 * g_*[n * row_stride + c] - so that SRCNNRes' folded backward (srcnn_res_arch.py:36-46) passes slices of its
 * (N, 9+P) constant-plane gradient without copying them out. */
int risp_stats_bwd_rows(float *gx, const float *g_min, const float *g_mean, const float *g_max,
                        const int32_t *arg, int N, int C, int HW, int row_stride, void *stream);

/* Per-plane histogram with torch.histc(x, bins, min=0, max=1) semantics (raw counts as fp32;
 * out-of-range values ignored; x == 1 in the last bin) - the conditional heads' feature,
 * tools_origin.py:120-128 (computed on the CPU there).  hist is (NC,bins), fully written. */
int risp_histc(const float *x, float *hist, int NC, int HW, int bins, void *stream);

/* SRCNNRes broadcast-plane values (srcnn_res_arch.py:36-43): cvals (N,9+P) =
 * [min_b,min_g,min_r | mean | max | pv (N,P)] from the stats of the (N,3,H,W) input. */
int risp_srcnn_cvals(const float *stats, const float *pv, float *cvals, int N, int P, int HW, void *stream);
/* the same values applied to a weight-only table: table (N,M) = cvals (N,9+P) @ rcase (9+P,M), terms in index order -
 * the per-(image, cout, border case) constants that replace the 9+P broadcast planes of SRCNNRes' 9x9 first layer
 * (srcnn_res_arch.py:41-46; M = 64 * 81, consumed by risp_conv2d with RISP_EPI_CASEBIAS). */
int risp_srcnn_case_table(const float *stats, const float *pv, const float *rcase, float *table, int N, int P, int HW,
                          int M, void *stream);

/* whitebalance 'grayworld' - tools_origin.py:33-41 ("output is clipped to [0, 1]", :22).
 * OPSPEC: gains[n,c] = gray_n / max(mean[n,c],1e-6), gray = mean over c of the channel means;
 * y = clamp(x * gains).  Composition: risp_channel_stats -> risp_grayworld_gains_fwd ->
 * risp_gain3_fwd; backward: risp_gain3_bwd -> risp_grayworld_gains_bwd -> risp_stats_bwd. */
int risp_grayworld_gains_fwd(const float *stats, float *gains, int N, int HW, void *stream);
int risp_grayworld_gains_bwd(const float *stats, const float *g_gains, float *g_mean, int N, int HW,
                             void *stream);
/* y[n,c] = clamp(x[n,c] * k[n,c], 0, 1); k is (N,3) */
int risp_gain3_fwd(const float *x, const float *k, float *y, int N, int HW, void *stream);
int risp_gain3_bwd(const float *x, const float *k, const float *gy, float *gx, float *gk, float *scratch, int N,
                   int HW, void *stream);

/* ---------------------------------------------------------------------------
 * Fused element-wise segment of a fixed pipeline (isp_universal.py:210-232): one
 * launch reads the segment input once and writes EVERY stage output
 * (intermediate_results is API).  ops[k] in RISP_OP_*; params[k] = (N,P_k) or NULL;
 * outs[k] = (N,3,H,W) (NULL for RISP_OP_SKIP, which aliases its input).
 * The first op may be RISP_OP_DEMOSAIC_NEAREST (input (N,1,H,W)); all others take BGR.
 * ------------------------------------------------------------------------- */
enum {
    RISP_OP_SKIP = 0,
    RISP_OP_DEMOSAIC_NEAREST = 1,
    RISP_OP_WB_MANUAL = 2,
    RISP_OP_GAMMA = 3,
    RISP_OP_GTM_MANUAL = 4,
    RISP_OP_WB_QUADRATIC = 5,
    RISP_OP_GAIN3 = 6, /* y_c = clamp(x_c * p[n,c]): gray-world apply with precomputed gains */
    /* the two classical tone curves that need no whole-image quantity: stages of risp_serve_classical_u8 ONLY (every other
     * entry point refuses codes above RISP_OP_GAIN3) */
    RISP_OP_TONE_CRYSIS = 7, /* params (N,1): lum_adapted */
    RISP_OP_TONE_FILMIC = 8  /* params (N,2): white_point, exposure_bias (already scaled to 1 .. 10) */
};
#define RISP_MAX_CHAIN 8
int risp_chain_fwd(const float *in, int n_ops, const int *ops, const float *const *params,
                   float *const *outs, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------
 * Mixed-op combiner (super_prune_fifteen_demos_four_bayer_two.py:183-212):
 * y = sum_k w[k] * o_k  over K op outputs of one slot (w = pruned, renormalised probs,
 * host array).  bwd: go_k = w[k]*gy (written only where go[k] != NULL) and
 * gw[k] = <gy, o_k> (device, K floats, fully written).
 * numel % 4 == 0; every o_k, go[k], gy and y 16-byte aligned (both kernels walk them in
 * 16-byte vectors): anything else is refused before a launch.
 * ------------------------------------------------------------------------- */
#define RISP_MAX_MIX 16
int risp_mix_fwd(const float *const *outs, const float *w, int K, float *y, size_t numel, void *stream);
/* scratch: risp_mix_scratch_floats() floats (one partial row per workgroup, added in index order: bit-repeatable) */
size_t risp_mix_scratch_floats(void);
int risp_mix_bwd(const float *const *outs, const float *w, int K, const float *gy,
                 float *const *go, float *gw, float *scratch, size_t numel, void *stream);

/* The mixture of a slot with its ELEMENT-WISE operators computed on the fly: operand k of y = sum_k w[k] o_k is either a
 * materialised (N,3,H,W) tensor (kind RISP_SLOT_TENSOR, ptr = the tensor: the CNN proxies) or o_k = op(x, params) for
 * kind RISP_OP_SKIP / WB_MANUAL / GAMMA / GTM_MANUAL / WB_QUADRATIC / GAIN3 (ptr = the (N,P) parameter block; at most one
 * operand of each kind) evaluated in registers from the slot input x: x is read once and the operators' outputs never
 * touch HBM.  pmul[k] multiplies a WB_MANUAL block on the way in (the wrapper's params * 5, tools_origin.py:214) and its
 * gradient on the way out.  y is bit-identical to running the operators one by one and risp_mix_fwd.
 * Backward: gw (K) = <gy, o_k>; go[k] (tensor operands, may be NULL) = w[k] gy; gx = sum over the element-wise operands of
 * their input gradients at upstream w[k] gy, added in KIND order (skip, manual white balance, gamma, tone curve, quadratic
 * white balance, gain - whatever the operand order; NULL allowed only when there is none); gp[k] = (N,P) parameter-gradient
 * block of operand k (GTM_MANUAL: whole batch in row 0), fully written, may be NULL.  Deterministic.  Identical bits to the
 * unfused slot: y, gp (and go); gw and gx differ from it by summation order (~1e-7). */
#define RISP_SLOT_TENSOR (-1)
#define RISP_SLOT_ROW (RISP_MAX_MIX + 40)
typedef struct risp_slot_mix_desc {
    int K, N, HW;
    int kind[RISP_MAX_MIX];
    float w[RISP_MAX_MIX], pmul[RISP_MAX_MIX];
    const float *ptr[RISP_MAX_MIX];
    float *go[RISP_MAX_MIX];                      /* backward */
    float *gp[RISP_MAX_MIX];                      /* backward */
    const float *x;
    float *y;                                     /* forward */
} risp_slot_mix_desc;
int risp_slot_mix_fwd(const risp_slot_mix_desc *d, void *stream);
size_t risp_slot_mix_scratch_floats(int N, int HW);
int risp_slot_mix_bwd(const risp_slot_mix_desc *d, const float *gy, float *gx, float *gw, float *scratch, void *stream);

/* ---------------------------------------------------------------------------
 * Convolution layers of the learned proxies on fp32 MFMA
 * (srcnn_res_arch.py:15-24, srcnn_demosaic_arch.py:14-25, path_14l_*_arch.py:6-57).
 * Stride 1, 'same' zero padding, odd square kernels.
 *
 *   y = epilogue( conv(load(x), W) + bias )
 *
 * wpack: weights repacked on the device by risp_conv_pack_weights into the
 * [chunk][tap][ci][cout_pad] slabs the kernel stages in LDS.
 * ------------------------------------------------------------------------- */
enum { /* how the kernel reads its input tensor */
    RISP_LOAD_PLAIN = 0,      /* x is (N,cin,H,W) */
    RISP_LOAD_UNSHUFFLE2 = 1, /* x is (N,cin/4,2H,2W); plane 4c+2i+j = x[c][2y+i][2x+j].  cin=4: the
                                 Bayer -> [R,G1,G2,B] split (path_14l_bayer_arch.py:70-75); also the
                                 backward of a PixelShuffle(2) store */
    RISP_LOAD_CONSTCH = 2     /* channels >= cin_img are per-image constants cvals[n,ci-cin_img]
                                 inside the image and 0 in the padding (SRCNNRes broadcast planes,
                                 srcnn_res_arch.py:41-46) */
};
enum { /* epilogue flags */
    RISP_EPI_RELU = 1,       /* y = max(y,0) */
    RISP_EPI_ADD = 2,        /* y[:, :add_c] += add (N,add_c,H,W), before the activation */
    RISP_EPI_MASK = 4,       /* y = (mask[n,co,h,w] > 0) ? y : 0   (backward through a ReLU) */
    RISP_EPI_SHUFFLE2 = 8,   /* store through PixelShuffle(2): (N,cout,H,W) -> (N,cout/4,2H,2W) */
    RISP_EPI_NOBIAS = 16,
    RISP_EPI_CASEBIAS = 32   /* y[n,co,h,w] += cvals[n,co,case(h),case(w)]: cvals is a (N,cout,k,k) table, case(v) = v
                                for v < k/2, k/2 in the interior, k-1-(L-1-v) for the last k/2 coordinates - the
                                contribution of spatially constant input channels (zero in the padding) folded out
                                of the layer: SRCNNRes broadcast planes, srcnn_res_arch.py:41-46.  Needs H,W >= k-1 */
};
typedef struct {
    int N, H, W;             /* H,W = conv resolution (half the source for RISP_LOAD_UNSHUFFLE2) */
    int cin, cout, ksize;    /* cout <= 64; ksize in {1,3,5,9} */
    int load_mode, cin_img;  /* cin_img: image channels when load_mode == RISP_LOAD_CONSTCH */
    int epilogue, add_c;
    const float *x, *wpack, *bias, *cvals, *add, *mask;
    float *y;
    /* Grouped launch (group_n = 0: off).  The same-geometry operators of a super-net slot - the 8 SRCNNRes proxies of an
     * sRGB slot, the 2 proxy demosaics (super_prune_fifteen_demos_four_bayer_two.py:35-52, looped at :183-212) - run each
     * layer as ONE launch: the N images are N / group_n consecutive groups of group_n images, group g convolves with
     * wpack + g * wpack_gs and bias + g * bias_gs (floats); y, mask, cvals (and x, add unless shared) are the groups'
     * tensors stacked along N.  RISP_GROUP_SHARED_X / _ADD: x / add hold ONE group's group_n images, read by every
     * group (the slot input).  Per image the arithmetic is that of the ungrouped launch: results are bit-identical. */
    int group_n, group_flags;
    long long wpack_gs, bias_gs;
} risp_conv_desc;
enum { RISP_GROUP_SHARED_X = 1, RISP_GROUP_SHARED_ADD = 2 };
size_t risp_conv_wpack_floats(int cin, int cout, int ksize);
/* w: device (cout,cin,k,k) torch layout.  transpose=1: w is the FORWARD layer's (cin,cout,k,k)
 * tensor and the pack holds the backward-data convolution (roles swapped, taps rotated 180). */
int risp_conv_pack_weights(const float *w, int cin, int cout, int ksize, int transpose, float *wpack,
                           void *stream);
int risp_conv2d(const risp_conv_desc *d, void *stream);

/* The same operator for layers with cout <= 12 (SRCNNRes conv 5x5 32->3, srcnn_res_arch.py:22; backward-data of its
 * 9x9 first layer :18 restricted to the 3 image channels; Path-Restore tails; SRCNNDemosaic conv 5x5 32->12,
 * srcnn_demosaic_arch.py:21): a direct vector-FMA kernel - the matrix-core kernel above pads cout to 32.
 * wpack: [cin][k][k][P] floats, P = risp_conv_small_cout_pad(cout) = 4 or 12 (couts zero-padded), 16-byte
 * aligned - the layer's weights w[co][ci][ky][kx] for a forward layer, w[ci_b][co_b][k-1-ky][k-1-kx] for a
 * backward-data layer.  cout == 3 (every proxy tail): [cin][k + 1][k][4] = (w0, w1, w2[ky], w2[ky - 1]) with w2[-1] = 0 and
 * row k = (0, 0, 0, w2[k - 1]) - the fourth lane of the packed FMAs then serves the third cout of a second output row.  load_mode PLAIN; epilogue RELU | ADD | MASK | NOBIAS, or SHUFFLE2 [| NOBIAS] with cout % 4 == 0;
 * ksize in {3,5,9} (9 only for cout <= 4). */
int risp_conv_small_cout_pad(int cout);
size_t risp_conv_small_wpack_floats(int cin, int cout, int ksize);
int risp_conv2d_small(const risp_conv_desc *d, void *stream);
/* Small grids (the per-GPU batch of the 8-GPU search is 4 images): the input channels are split over `groups`
 * workgroups per tile, partial sums go to scratch (groups * N * cout * H * W floats) and a second launch adds them
 * in index order and applies the epilogue (deterministic).  risp_conv_small_groups: the split worth using (1 = none). */
int risp_conv_small_groups(const risp_conv_desc *d);
int risp_conv2d_small_split(const risp_conv_desc *d, float *scratch, int groups, void *stream);

/* The same operator for 3x3 layers with a one-dimensional Winograd transform F(4,3) along x, fp32 throughout (half the
 * matrix-core work of risp_conv2d; Path-Restore's 64->64 layers, path_14l_bayer_arch.py:6-21, when RISP_CONV_ARITH=f32):
 * wpack [cout block of 32][chunk of risp_conv_wino43_chunk() cin][ky][t][ci][32], U_t = (G g)_t, G rows (1/4,0,0)
 * (1/6,1/6,1/6) (1/6,-1/6,1/6) (1/24,1/12,1/6) (1/24,-1/12,1/6) (0,0,1) applied to filter row g = w[co][ci][ky][0..2]
 * (backward-data: the forward weight with roles swapped and taps rotated by 180 degrees).  load_mode PLAIN, W % 4 == 0,
 * 16-byte aligned tensors, cout <= 64; epilogue RELU | ADD | MASK | NOBIAS; no grouped launches.  Layers with 33..64 couts
 * and cin % 4 == 0 run both cout blocks in one wave (same results bit for bit).  The library reads no environment. */
int risp_conv_wino43_chunk(void);
size_t risp_conv_wino43_wpack_floats(int cin, int cout);
int risp_conv2d_wino43(const risp_conv_desc *d, void *stream);

/* The same operator for 5x5 layers with at most 3 INPUT channels and 32 or 64 output channels in split precision on the f16 matrix
 * pipe (round 6, risp_conv_thin5.hip): the backward-data pass of SRCNNRes' last layer (srcnn_res_arch.py:22 - the upstream gradient's 3
 * image channels -> 32 hidden channels, masked by the ReLU of the layer before, :20), which the fp32 Winograd kernel served at 4 padded
 * channels.  Reduction index of a matrix instruction = (filter row, channel): 15 of 16 slots; the filter column shifts the pixel operand.
 * wpack (risp_conv_thin5_wpack_bytes(cout) bytes, 16-byte aligned): a 16-byte header whose first float is 1 / s_w, then [cout block of
 * 32][kx][part: hi, lo][half of the reduction index][cout][8] halves of w * s_w, reduction index k = 3 ky + c (k = 15 and missing
 * channels zero) - the layer's weights w[co][c][ky][kx] (backward-data: the forward weight with roles swapped and taps rotated by 180
 * degrees).  load_mode PLAIN; epilogue RELU | MASK | NOBIAS; cout * H * W * 4 < 2^31; any W; grouped launches.  One scale per work item
 * (image, 128-column strip, 32-row segment): a result does not depend on the batch; every sum in a fixed order. */
size_t risp_conv_thin5_wpack_bytes(int cout);
int risp_conv2d_thin5(const risp_conv_desc *d, void *stream);

/* The same operator for 3x3 layers with at most 4 OUTPUT channels and 16 .. 64 input channels (a multiple of 16) in split precision on
 * the f16 matrix pipe (round 6, risp_conv_narrow3.hip): Path-Restore's last layer (path_14l_bgr_arch.py, path_14l_bayer_arch.py: 64 -> 3,
 * 64 -> 4 + PixelShuffle) and the backward-data pass of its first layer.  Rows of a matrix instruction = (filter row, cout), reduction
 * index = 16 channels, the filter column shifts the pixel operand; a wave walks down the rows and the three filter rows' contributions
 * meet in registers.  wpack (risp_conv_narrow3_wpack_bytes(cin) bytes, 16-byte aligned): a 16-byte header whose first float is 1 / s_w,
 * then [chunk of 16 cin][kx][part: hi, lo][channel half][row m, 32][8 channels] halves of w * s_w, row m = 4 ky + co (other rows zero) -
 * the layer's weights w[co][ci][ky][kx] (backward-data: the forward weight with roles swapped and taps rotated by 180 degrees).
 * load_mode PLAIN; epilogue RELU | SHUFFLE2 (cout == 4) | NOBIAS; cin * H * W * 4 < 2^31; any W; grouped launches.  One scale per wave
 * and input row: a result depends neither on the batch nor on how the launch cuts its row segments; every sum in a fixed order. */
size_t risp_conv_narrow3_wpack_bytes(int cin);
int risp_conv2d_narrow3(const risp_conv_desc *d, void *stream);

/* The same operator for the FIRST layers of the proxies - few input channels, the whole weight matrix staged once per
 * workgroup - with a LINEAR reduction index k = (ci * ksize + ky) * ksize + kx, so that the matrix instruction's two k-slots
 * hold consecutive k (3 channels of a 9x9 layer: 122 instructions per tile instead of the 162 that channel PAIRS cost in
 * risp_conv2d):  9x9 3 -> cout (SRCNNRes with its broadcast planes folded out, srcnn_res_arch.py:18, 41-46), 3x3 3 -> cout
 * (path_14l_bgr_arch.py:40-43) with load_mode PLAIN;  9x9 4 -> cout (srcnn_demosaic_arch.py:14-16, 39-43) and 3x3 4 -> cout
 * (path_14l_bayer_arch.py:37-40, 70-75) with load_mode UNSHUFFLE2 (x = the (N,1,2H,2W) mosaic).  cout <= 64.
 * wpack: [cout block][2 ceil(cin k k / 2)][B] floats, B = risp_conv_k3_cout_block(cin, ksize) (32 or 64), entry [b][k][c] =
 * w[b B + c][ci][ky][kx], zero beyond the layer, 16-byte aligned.  W % 4 == 0, 16-byte aligned tensors; epilogue RELU |
 * NOBIAS | CASEBIAS. */
int risp_conv_k3_cout_block(int cin, int ksize);
size_t risp_conv_k3_wpack_floats(int cin, int cout, int ksize);
int risp_conv2d_k3(const risp_conv_desc *d, void *stream);

/* 5x5 layers with F(4,5) along x (0.4 of the matrix-core work of risp_conv2d; SRCNNRes' 64->32 layer and its backward,
 * srcnn_res_arch.py:20, when RISP_CONV_ARITH=f32, and the 5x5 backward passes with 3 or 12 input channels): U_t = (G g)_t / s_t,
 * G rows (1,0,0,0,0) (1,1,1,1,1) (1,-1,1,-1,1) (1,2,4,8,16) (1,-2,4,-8,16) (1,1/2,1/4,1/8,1/16) (1,-1/2,1/4,-1/8,1/16)
 * (0,0,0,0,1), s = (1, -18, -18, 360, 360, 45/16, 45/16, 1), applied to filter row g = w[co][ci][ky][0..4].  wpack (layout 1,
 * what risp_conv_wino45_layout() returns): [cout block of 32][chunk of 4 cin][ky][point group 2][cout block of 16: 2][ci 4]
 * [cout 16][4 points] (two output rows per wave).  cin % 4 == 0 or cin < 4; otherwise the restrictions of risp_conv2d_wino43;
 * grouped launches. */
int risp_conv_wino45_chunk(void);
int risp_conv_wino45_layout(void);
size_t risp_conv_wino45_wpack_floats(int cin, int cout);
int risp_conv2d_wino45(const risp_conv_desc *d, void *stream);

/* The same operator on the f16 matrix pipe at fp32-level accuracy (round 4; the 64 -> 64 3x3 layers of Path-Restore,
 * path_14l_bgr_arch.py:6-21, 58-86; path_14l_bayer_arch.py:59-88; the 5x5 64 -> 32 layer of SRCNNRes and its backward,
 * srcnn_res_arch.py:20): every fp32 operand is cut into two f16 halves,
 * hi = rn_f16(v s), lo = rn_f16(v s - hi), and x w is taken as (x_lo w_hi + x_hi w_lo + x_hi w_hi) / (s_x s_w) - three
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation instead of eight fp32 matrix instructions of twice the duration; the
 * dropped term is 2^-22 of the product.  x, y, add, mask stay fp32 tensors: the activations are scaled (per workgroup tile
 * and chunk of 16 input channels, by the tile's own largest magnitude - so gradients of magnitude 1e-8 are as exact as
 * activations of magnitude 1) and split at staging time; the weights are scaled and split once, at pack time.
 * wpack: risp_conv_f16x2_wpack_bytes() bytes, 16-byte aligned: a 16-byte header whose first float is 1 / s_w (s_w = 2^k with
 * max|w| s_w in [2^14, 2^15)), then [chunk of 16 cin][tap][part: hi, lo][channel half][cout padded to 32 or 64][8 channels]
 * _Float16 (reconfigisp_amd/convnets.py::f16x2_weights).  ksize 3 or 5, cin % 16 == 0, cout 32 or 64, add_c == cout, W % 4 == 0,
 * max(cin, cout) * H * W * 4 < 2^31 bytes per image, 16-byte aligned tensors, load_mode PLAIN; epilogue RELU | ADD | MASK | NOBIAS; grouped
 * launches (group_n, strides in floats).  A tile's result does not depend on the batch it travels in. */
size_t risp_conv_f16x2_wpack_bytes(int cin, int cout, int ksize);
int risp_conv2d_f16x2(const risp_conv_desc *d, void *stream);
/* The same layer, same pack, same bits by the form risp_conv2d_f16x2 had in round 4: two 4-wave workgroups per CU in which every
 * wave stages, waits and multiplies (risp_conv2d_f16x2 = one 8-wave workgroup per CU, four waves stage tiles and weights a chunk
 * ahead, four issue the matrix instructions).  Serves the one-chunk 3x3 64-cout shape the wave-specialised form does not take;
 * tests/test_gpu_f16x2.py holds the two to identical bits on every shape and epilogue.  The library keeps no switch between them. */
int risp_conv2d_f16x2_uniform(const risp_conv_desc *d, void *stream);

/* The same arithmetic for layers with at most 4 output channels and a 5- or 9-tap filter row (round 4; SRCNNRes conv 5x5 32 -> 3,
 * srcnn_res_arch.py:22; backward-data of its 9x9 first layer restricted to the 3 image channels, :18; backward-data of
 * SRCNNDemosaic's 9x9 4 -> 64 through PixelShuffle, srcnn_demosaic_arch.py:14-16): the rows of the matrix instruction are
 * (cout, position j inside a block of 8 pixels), its columns the 32 blocks of a 256-pixel row, its reduction index a window of 16
 * input pixels of one input channel and filter row - a Toeplitz band of the filter row as the A operand.
 * wpack: risp_conv_toep_wpack_bytes() bytes, 16-byte aligned: a 16-byte header whose first float is 1 / s_w, then
 * [cin][ky][part: hi, lo][window half][row m = 8 cout + j, padded to 32][8 window slots] _Float16 with
 * band[m][u] = w[co][ci][ky][u - j + k/2 - 4] s_w (0 outside the filter row; reconfigisp_amd/convnets.py::toep_weights).
 * cout <= 4 (ksize 9 or 5), or 5 .. 12 with ksize 5 (SRCNNDemosaic's 5x5 32 -> 12 tail, srcnn_demosaic_arch.py:21: three row blocks,
 * rows padded to 96); any cin, W % 4 == 0, fewer than 2^30 input elements per image, 16-byte aligned tensors, load_mode PLAIN;
 * epilogue RELU | ADD (add_c <= cout) | NOBIAS, or SHUFFLE2 [| NOBIAS] with cout % 4 == 0; grouped launches. */
size_t risp_conv_toep_wpack_bytes(int cin, int cout, int ksize);
int risp_conv2d_toep(const risp_conv_desc *d, void *stream);
/* The same launch also writing, per tile of 16 rows x 256 columns, the sum of every input channel over the tile's own pixels:
 * psum [N][risp_conv_toep_tiles(H, W)][cin] floats.  risp_rect_sums_tiles (below, next to risp_rect_sums) finishes them into the
 * rectangle sums of SRCNNRes' constant planes (srcnn_res_arch.py:41-46) from the border rows and columns alone - the 64-channel
 * upstream gradient is read once, by the backward-data convolution. */
int risp_conv_toep_tiles(int H, int W);
int risp_conv2d_toep_sums(const risp_conv_desc *d, float *psum, void *stream);

/* The layers with at most 3 output channels and cin % 16 == 0 (SRCNNRes conv 5x5 32 -> 3 forward, srcnn_res_arch.py:22; backward-data of
 * its 9x9 first layer restricted to the 3 image channels, :18) with the filter ROWS moved into the rows of the matrix instruction
 * (round 6, risp_conv_tapout.hip): reduction index = 16 input channels (dense), rows = (cout, ky), the filter column kx = a shift of the
 * pixel operand; one matrix pass per INPUT row, whose 3 x k results are added into a ring of output rows (every address by one lane
 * in program order: bit-repeatable).  Half the matrix instructions of risp_conv2d_toep for 9x9 64 -> 3.  Split precision as in
 * risp_conv2d_f16x2, activations scaled per (4 rows x 136 columns, 16 channels).
 * wpack: risp_conv_tapout_wpack_bytes() bytes, 16-byte aligned: a 16-byte header whose first float is 1 / s_w, then [chunk of 16
 * cin][kx][part: hi, lo][channel half][row m, 32][8 channels] _Float16 with row m = 4 ky + co (ky < 8) or 4 co + 3 (ky = 8)
 * (reconfigisp_amd/convnets.py::tapout_weights).  ksize 5 or 9, cout <= 3, cin % 16 == 0, W % 4 == 0, H * W < 2^24, cin * H * W < 2^30;
 * load_mode PLAIN; epilogue RELU | ADD (add_c <= cout) | NOBIAS; grouped launches.  seg_rows: rows of a work item's segment - 0 = chosen by the launch to fill
 * the chip (training launches), else fixed by the caller - a multiple of 4 (the scales follow the segment's row phase), or any value of at
 * least H (the image kept whole: what risp_conv_tapout_seg_rows returns for a launch it does not cut, whatever H % 4): an image's result
 * then does not depend on the batch it travels in. */
size_t risp_conv_tapout_wpack_bytes(int cin, int ksize);
int risp_conv_tapout_seg_rows(int N, int H, int W);          /* what seg_rows = 0 chooses for a launch of N images (a pure function) */
int risp_conv2d_tapout(const risp_conv_desc *d, int seg_rows, void *stream);
/* ... and, on the way, the sum of every input channel over every work item's own pixels (ksize 9, cin 64):
 * psum [N][risp_conv_tapout_items(N, H, W, seg_rows)][64] floats, finished by risp_rect_sums_tiles. */
int risp_conv_tapout_items(int N, int H, int W, int seg_rows);
int risp_conv2d_tapout_sums(const risp_conv_desc *d, int seg_rows, float *psum, void *stream);

/* ... and for the 9x9 FIRST layers (few input channels, 64 couts: SRCNNRes 3 -> 64 with its broadcast planes folded out,
 * srcnn_res_arch.py:18, 41-46; SRCNNDemosaic 4 -> 64 on the mosaic, srcnn_demosaic_arch.py:14-16, 39-43 - what risp_conv2d_k3
 * does on the fp32 matrix pipe): rows = 32 couts, one accumulator per pixel position j of a block of 8, the 8 A operands are
 * windows of one zero-padded filter row per lane.  wpack: risp_conv_toep_first_wpack_bytes() bytes, 16-byte aligned: a 16-byte
 * header whose first float is 1 / s_w, then [cout block of 32][cin][ky][part: hi, lo][taps 0-7 | tap 8 and 7 zeros][cout][8] _Float16
 * (reconfigisp_amd/convnets.py::toep_first_weights).  ksize 9, cin <= 16, W % 4 == 0, 16-byte aligned tensors; load_mode PLAIN, or
 * UNSHUFFLE2 with cin == 4 (x = the (N,1,2H,2W) mosaic); epilogue RELU | NOBIAS | CASEBIAS; grouped launches. */
size_t risp_conv_toep_first_wpack_bytes(int cin, int cout);
int risp_conv2d_toep_first(const risp_conv_desc *d, void *stream);
/* ... with exact ReLU decisions, for training forwards: outputs whose pre-activation lies within the arithmetic's own error of zero
 * (|z| < 2^-20 x 81 x max|w| x the tile's input magnitude summed over the channels) are listed in `ties` ([0] = count, then up to
 * max_ties linear output indices; cleared by this call) and a second launch recomputes them in double - exact products, fixed
 * order, one rounding - from the layer's fp32 weights w32 (cout,cin,9,9), the members of a grouped launch w32_gs floats apart.
 * Fewer than 2^32 outputs.  Which way such an activation falls otherwise depends on the summation order of whichever fp32-accurate
 * kernel computed it, and one ReLU mask bit is a finite step of every gradient behind it.  (Opt-in: RISP_CONV_TOEP_FIRST=train.) */
int risp_conv2d_toep_first_exact(const risp_conv_desc *d, const float *w32, long long w32_gs, unsigned *ties, unsigned max_ties,
                                 void *stream);

/* out[p][ky][kx] = sum of g[p] (planes x H x W) over the pixels q with q + (ky - k/2, kx - k/2) inside the plane:
 * what the backward of a k x k convolution over a spatially CONSTANT input channel needs from the upstream gradient
 * (d loss / d constant = sum_{co,tap} w[co][c][tap] * out[co][tap]).  k odd <= 9, H, W >= k/2. */
int risp_rect_sums(const float *g, float *out, int planes, int H, int W, int ksize, void *stream);
/* out as risp_rect_sums with ksize 9, from psum [N][tiles][C] (risp_conv2d_toep_sums) and the 4 border rows / columns of the planes
 * g (N,C,H,W); H, W >= 4, W % 4 == 0.  Another summation order than risp_rect_sums (agreement ~1e-6 of the plane's sum). */
int risp_rect_sums_tiles(const float *g, const float *psum, float *out, int N, int C, int H, int W, int tiles, void *stream);
/* ... and that product: gconst (N,C) = rs (N,M) @ wconst (M,C) (SRCNNRes: M = 64 * 81 rectangle sums per
 * image, C = 9+P constant planes, srcnn_res_arch.py:41-46).  Deterministic. */
int risp_srcnn_const_grad(const float *rs, const float *wconst, float *gconst, int N, int M, int C, void *stream);

/* ---------------------------------------------------------------------------
 * The same-geometry proxies of a super-net slot as ONE launch per layer (the 8 SRCNNRes of an sRGB slot,
 * super_prune_fifteen_demos_four_bayer_two.py:35-52 / :183-212; srcnn_res_arch.py:15-53).  The convolutions use
 * risp_conv_desc.group_n; these are the non-convolution links of the chain for all members at once.  Member g has P[g]
 * parameter channels; tensors of the group are the members' tensors stacked along N (member-major: row g * N + n).
 * Per member every value is computed exactly as by the single-operator entry point named beside it.
 * ------------------------------------------------------------------------- */
#define RISP_MAX_GROUP 16
typedef struct risp_srcnn_group_desc {
    int G, N, HW, M;                              /* members, images per member, H*W, table width (cout * k * k) */
    int P[RISP_MAX_GROUP];
    const float *pv[RISP_MAX_GROUP];              /* (N, P[g]) parameter blocks (forward) */
    const float *rcase[RISP_MAX_GROUP];           /* (9 + P[g], M) folded first-layer tables (forward) */
    const float *wconst[RISP_MAX_GROUP];          /* (M, 9 + P[g]) constant-plane weights (backward) */
} risp_srcnn_group_desc;
/* table (G*N, M): risp_srcnn_case_table per member; stats (N,3,4) of the shared input */
int risp_srcnn_case_table_group(const float *stats, const risp_srcnn_group_desc *d, float *table, void *stream);
/* gconst (G*N, row), row >= max(9 + P): risp_srcnn_const_grad per member into columns [0, 9 + P[g]), zeros beyond */
int risp_srcnn_const_grad_group(const float *rs, const risp_srcnn_group_desc *d, float *gconst, int row, void *stream);
/* out (N,C,H,W) = sum over the members, in member order, of stack (G,N,C,H,W).  gstats != NULL: member g's term first
 * receives risp_stats_bwd_rows with g_min / g_mean / g_max = columns [0,C) / [C,2C) / [2C,3C) of gstats (G*N, row) and
 * the argmin / argmax indices `arg` (N,C,2) of the shared input. */
int risp_group_sum(const float *stack, float *out, int G, int N, int C, int HW, const float *gstats, int row,
                   const int32_t *arg, void *stream);

/* Backward-weight of the same layer: dw (cout,cin,k,k) = sum_{n,y,x} gy[n,co,y,x] * load(x)[n,ci,y+ky-p,x+kx-p]
 * (fully written).  Uses d->x, load_mode (PLAIN / CONSTCH), cin_img, cvals, N, H, W, cin, cout, ksize; gy is
 * (N,cout,H,W).  scratch: scratch_floats >= risp_conv_wgrad_scratch_floats(cin, cout, ksize) floats, checked (per-workgroup partial sums:
 * 768 slices of the pixel tiles, dealt over the 32 x 32 blocks of (cout, cin), k * k slots each - k for the thin layers whose filter column
 * is packed into the matrix -, added in index order by a finishing launch - no atomics, the same bits on every run).
 * Limits: cin and cout 1 .. 64 and ksize 1, 3, 5 or 9, but ksize 9 only with cin <= 31 - the tiles of 32 input channels and more
 * (32 x 129 + 32 x 385 floats = 65 792 bytes) are past the 64 KiB of LDS a workgroup may ask for, whatever cout ("tile too large
 * for LDS").  The bias gradient is not part of this entry: convnets.conv_wgrad takes it from risp_plane_sums, which holds
 * N * cout <= 65535.  Refusals return before any launch and write nothing (tests/test_gpu_wgrad_space.py).
 * Only the proxy fine-tuning path (darts_ft_model.py:206-246) needs weight gradients. */
size_t risp_conv_wgrad_scratch_floats(int cin, int cout, int ksize);
int risp_conv2d_wgrad(const risp_conv_desc *d, const float *gy, float *dw, float *scratch, size_t scratch_floats, void *stream);

/* sum over H,W of channels [c0, c0+nc) of an (N,C,H,W) tensor -> out (N,nc) (SRCNNRes
 * gradient of the broadcast parameter planes).  16-byte loads where HW % 4 == 0 and x is 16-byte
 * aligned, element loads otherwise (as risp_channel_stats). */
int risp_plane_sums(const float *x, float *out, int N, int C, int c0, int nc, int HW, void *stream);

/* ---------------------------------------------------------------------------
 * Conditional modules (sRGB pool 16-18): the fully connected head, ConditionalModuleBGR._fc_forward
 * (tools_origin.py:109-163).  hist (N, widths[0]) raw histogram counts (risp_histc; no gradient);
 * flat: per layer an (in,out) row-major weight then a bias, then the "global" block whose FIRST entry is
 * added to every output unit (:158-160); ReLU between layers, sigmoid at the end.
 * acts / deltas: (N, risp_cond_fc_row_floats) scratch rows kept by the caller between forward and backward.
 * out (N, widths[n_layers]); dflat (total_params) is fully written (deterministic, no atomics).
 * ------------------------------------------------------------------------- */
int risp_cond_fc_row_floats(const int *widths, int n_layers);
int risp_cond_fc_fwd(const float *hist, const float *flat, const int *widths, int n_layers, float *acts, float *out, int N,
                     void *stream);
int risp_cond_fc_bwd(const float *flat, const int *widths, int n_layers, const float *acts, const float *out, const float *gout,
                     float *deltas, float *dflat, int total_params, int N, void *stream);

/* ---------------------------------------------------------------------------
 * Bookkeeping of one super-net slot as single launches (models/modules/super_prune_fifteen_demos_four_bayer_two.py).
 * ------------------------------------------------------------------------- */
/* mixture weights, :185-193: prob = softmax(alpha) (entries flagged in `unavailable` get probability exactly 0);
 * entries with prob < threshold * max(prob) (strict) are pruned; post = kept / sum(kept).  The mask and the sum are
 * detached in the reference, so d post_k / d prob_k = coef_k (1 / sum for kept entries, 0 for pruned ones).
 * K <= 64.  probs, coef, post: K floats each (probs and coef feed the backward). */
int risp_prune_softmax_fwd(const float *alpha, const unsigned char *unavailable, float threshold, int K, float *probs,
                           float *coef, float *post, void *stream);
int risp_prune_softmax_bwd(const float *probs, const float *coef, const float *gpost, int K, float *galpha, void *stream);

/* per-image parameter blocks of the ops of a slot, :204-209 / isp_universal.py:226-228:
 * block[k] (N, width[k]) = sigmoid(raw[k]).repeat(N, 1); backward: graw[k] = sigmoid' * sum over the images of
 * gblock[k] (NULL = no gradient arrived: zeros), images in index order (deterministic). */
#define RISP_MAX_PARAM_OPS 16
typedef struct risp_param_blocks_desc {
    int n_ops, N;
    int width[RISP_MAX_PARAM_OPS];                /* 1..64 */
    const float *raw[RISP_MAX_PARAM_OPS];         /* (width) */
    float *block[RISP_MAX_PARAM_OPS];             /* forward: (N, width) out */
    const float *gblock[RISP_MAX_PARAM_OPS];      /* backward: (N, width) in, may be NULL */
    float *graw[RISP_MAX_PARAM_OPS];              /* backward: (width) out */
    int gstride[RISP_MAX_PARAM_OPS];              /* backward: floats between the rows of gblock[k] (0 = width: packed) */
} risp_param_blocks_desc;
int risp_param_blocks_fwd(const risp_param_blocks_desc *d, void *stream);
int risp_param_blocks_bwd(const risp_param_blocks_desc *d, void *stream);

/* ---------------------------------------------------------------------------
 * The glue of a DARTS iteration as own launches (risp_step.hip).
 * ------------------------------------------------------------------------- */
/* loss[0] = mean((y - gt)^2) (kind 0: nn.MSELoss, models/darts_model.py:58-63, isp_model.py:29-34) or mean(|y - gt|) (kind 1:
 * nn.L1Loss) over numel values, numel % 4 == 0, 16-byte aligned; g != NULL: also the gradient of that mean with respect to y
 * at upstream 1 (2 (y - gt) / numel, sign(y - gt) / numel) - the backward pass is then a scaling.  Two launches (partial sums
 * per workgroup into scratch = risp_loss_scratch_floats() floats, added in index order): deterministic. */
size_t risp_loss_scratch_floats(void);
int risp_pixel_loss(const float *y, const float *gt, float *g, float *loss, float *scratch, size_t numel, int kind, void *stream);

/* local_global_loss with the mean-squared loss (utils/util_loss.py:26-64, pixel_criterion local_global_l2): images with flag[n] < 1
 * ("local"): MSE of (a * gain, b), gain[n][c] = clamp(mean b / (clamp(mean a, 0) + 1e-6), 0.5, 2), no gradient through the gain; the
 * others ("global"): MSE of the 1/4-scale bilinear down-samples (align_corners false; H, W % 4 == 0); loss[0] = the sum of the two means
 * (an empty branch contributes 0), g (may be NULL) = d loss / d a.  flag (N) floats ON THE DEVICE: no host read, no boolean indexing.
 * scratch: risp_local_global_scratch_floats(N, C) floats; four launches, partial sums added in index order. */
size_t risp_local_global_scratch_floats(int N, int C);
int risp_local_global_l2(const float *a, const float *b, const float *flag, float *g, float *loss, float *scratch, int N, int C, int H, int W,
                         void *stream);

/* The reference's per-parameter Python loops over the <= 216 floats of a super-net as ONE launch over a table of tensors. */
#define RISP_MAX_LIST 64
typedef struct risp_list_desc {
    int n;                                        /* tensors, <= RISP_MAX_LIST */
    int numel[RISP_MAX_LIST];
    float *a[RISP_MAX_LIST];                      /* written */
    const float *b[RISP_MAX_LIST];
    const float *c[RISP_MAX_LIST];
    const float *e[RISP_MAX_LIST];
} risp_list_desc;
/* virtual step, darts_model.py:204-222: a = b - lr_meta * (momentum * e + c); e NULL: no momentum buffer yet; c NULL: a = b
 * (no gradient arrived, or an alpha copied to the twin network).  Operation by operation the reference's arithmetic. */
int risp_darts_virtual_step(const risp_list_desc *d, float momentum, float lr_meta, void *stream);
/* out[0] = 2-norm of the concatenation of the c[t] (NULL entries skipped), out[1] = eps = out[0] < 1e-6 ? 0 : 0.01 / out[0]
 * (:274-277); fixed summation order.  Lists longer than RISP_MAX_LIST go through risp_list_norm_eps_part in pieces: first = 0
 * continues from the sum of squares the previous piece left in out[0]; last = 0 leaves the running sum of squares there instead of
 * finishing (risp_list_norm_eps = one piece with first = last = 1). */
int risp_list_norm_eps(const risp_list_desc *d, float *out, void *stream);
int risp_list_norm_eps_part(const risp_list_desc *d, float *out, int first, int last, void *stream);
/* a[t] += (factor * scalar[0]) * c[t] (c NULL: untouched): the +eps, -2 eps, +eps shifts of the parameters (:299-312) with
 * eps on the device. */
int risp_list_axpy_scalar(const risp_list_desc *d, const float *scalar, float factor, void *stream);
/* The optimizers of the search (darts_model.py:78-81) over the table, in place, as torch.optim writes them (no weight decay,
 * dampening, nesterov, amsgrad): SGD with momentum - e = momentum buffers: e = first ? c : e * momentum + c; a -= lr * e - and
 * Adam - b = exp_avg, e = exp_avg_sq (both updated), lr_step = lr / (1 - beta1^t), bias2_sqrt = sqrt(1 - beta2^t),
 * one_minus_beta = (float)(1 - beta) formed in double like torch's lerp_ / addcmul_ weights.  The denominator is
 * sqrt(exp_avg_sq) / bias2_sqrt + eps with a true division (torch's list-wide CUDA form; its CPU form multiplies by the
 * reciprocal: 1 ulp apart).  Rows whose gradient c is NULL are left alone. */
int risp_sgd_momentum_step(const risp_list_desc *d, float lr, float momentum, int first, void *stream);
int risp_adam_step(const risp_list_desc *d, float lr_step, float beta2, float one_minus_beta1, float one_minus_beta2, float bias2_sqrt,
                   float eps, void *stream);
/* architecture gradient, :254-265 with :313-323: a = b - lr_meta * ((c - e) / 2 * eps[0]); zeros where b, c or e is NULL or
 * the finite-difference term holds a NaN (nan_flags[t] = 1 there; may be NULL).  numel <= 256. */
int risp_darts_alpha_grad(const risp_list_desc *d, const float *eps, float lr_meta, int *nan_flags, void *stream);

/* ---------------------------------------------------------------------------
 * One training step of an element-wise fixed pipeline in two launches - replaces the body of
 * IspModel.optimize_parameters (models/isp_model.py:128-142: output = netG(img); l_pix = cri_pix(output, gt);
 * zero_grad(); l_pix.backward(); optimizer_G.step()) when netG is [nearest demosaic ->] a chain of WbManual / Gamma /
 * GtmManual / WbQuadratic stages (isp_universal.py:210-232), cri_pix is nn.MSELoss or nn.L1Loss (mean) and
 * optimizer_G is torch.optim.Adam without weight decay / amsgrad.  Forward, loss, backward (stage inputs kept in
 * registers), the parameter-gradient reduction (deterministic), the chain rule through sigmoid(raw).repeat(N,1)
 * [* 5 for WbManual] and the Adam update all happen on the device; only in, gt and y touch HBM.
 * ------------------------------------------------------------------------- */
#define RISP_MAX_TRAIN_CHAIN 6
typedef struct risp_train_desc {
    const float *in;                              /* (N,1,H,W) RGGB mosaic if from_bayer, else (N,3,H,W) BGR */
    const float *gt;                              /* (N,3,H,W) */
    float *y;                                     /* (N,3,H,W) pipeline output (IspModel.output); may be NULL */
    int from_bayer;                               /* a nearest-neighbour demosaic (tools_origin.py:278-284) in front */
    int n_ops;                                    /* parametrised stages, 1..RISP_MAX_TRAIN_CHAIN */
    int ops[RISP_MAX_TRAIN_CHAIN];                /* RISP_OP_WB_MANUAL / GAMMA / GTM_MANUAL / WB_QUADRATIC (at most one) */
    float *blocks[RISP_MAX_TRAIN_CHAIN];          /* (N,P_k) per-image parameter blocks the stages read = sigmoid(raw)
                                                     .repeat(N,1) (x 5 for WbManual); REWRITTEN for the next step */
    float *raw[RISP_MAX_TRAIN_CHAIN];             /* (P_k) learnable vectors (param_step<k>_<name>): updated in place */
    float *grad[RISP_MAX_TRAIN_CHAIN];            /* (P_k) d loss / d raw: what .grad holds after backward() */
    float *exp_avg[RISP_MAX_TRAIN_CHAIN];         /* (P_k) Adam first moment, updated in place */
    float *exp_avg_sq[RISP_MAX_TRAIN_CHAIN];      /* (P_k) Adam second moment, updated in place */
    int loss_kind;                                /* 0 = nn.MSELoss, 1 = nn.L1Loss (mean reduction) */
    int N, H, W;                                  /* H, W even */
    float lr_step;                                /* lr / (1 - beta1^t), t = this step's number (1-based) */
    float beta1, beta2;
    float one_minus_beta1, one_minus_beta2;       /* (float)(1 - beta): formed in double and rounded once, as torch forms the
                                                     weights of lerp_ / addcmul_ (1.f - 0.999f is 1.3e-5 off float(0.001)) */
    float bias2_sqrt;                             /* sqrt(1 - beta2^t) */
    float eps;
    float *loss;                                  /* 1 float: the mean loss of this step */
    float *scratch;                               /* risp_train_scratch_floats(N) floats */
} risp_train_desc;
size_t risp_train_scratch_floats(int N);
int risp_chain_train_step(const risp_train_desc *d, void *stream);

/* ---------------------------------------------------------------------------
 * Overlapped tiling (utils/util_path_restore.py:47-134), NCHW on device.
 * positions: host int32 [T][2] (y,x).
 * ------------------------------------------------------------------------- */
int risp_tile_gather(const float *img, float *patches, const int32_t *pos_dev, int T, int C,
                     int H, int W, int h, int w, void *stream);
int risp_tile_blend(const float *patches, float *img, const int32_t *pos_dev, int T, int C,
                    int H, int W, int h, int w, int eh, int ew, void *stream);
/* risp_tile_blend followed by risp_quantise_u8_flip in ONE launch, the fp32 frame never written: patches (T,C,h,w) fp32 and
 * pos_dev (T,2) int32 (y,x) as for risp_tile_blend, out (H,W,C) packed bytes, C 1 or 3.  Per pixel and channel the arithmetic
 * is risp_tile_blend's, expression for expression and in tile order - m = min(ramp_y, ramp_x), cnt += m, acc += p * m,
 * acc / cnt - and then risp_quantise_u8's: the product with 255 in fp32, clipped to [0,255], truncated.  reverse_channels as
 * in risp_quantise_u8.  flip (bit 0 x, bit 1 y: the RISP_CFA_* bits) stores the image un-mirrored, as risp_quantise_u8_flip
 * does: output pixel (Y,X) is blended pixel (fy ? H-1-Y : Y, fx ? W-1-X : X).  Contract, byte for byte:
 *     out == risp_quantise_u8_flip(risp_tile_blend(patches, ...), ..., reverse_channels, flip).
 * A thread owns four adjacent pixels of a row: 16-byte tile loads and three dword stores where W % 4 == 0, w % 4 == 0, patches
 * is 16-byte and out 4-byte aligned (a tile whose x origin is no multiple of 4 is read float by float inside the same launch);
 * every other geometry and alignment takes a scalar form with the same bytes.
 * Rules (anything else is refused before a launch and the message names the value): no NULL pointer; 1 <= T <= 65535; C 1 or
 * 3; 1 <= h <= H <= 65535, 1 <= w <= W; 0 <= eh <= h / 2, 0 <= ew <= w / 2; flip 0 .. 3.  Every tile lies inside the frame and
 * every pixel under a tile (the caller's part, as for risp_tile_blend). */
int risp_tile_blend_u8(const float *patches, uint8_t *out, const int32_t *pos_dev, int T, int C,
                       int H, int W, int h, int w, int eh, int ew, int reverse_channels, int flip, void *stream);

/* ---------------------------------------------------------------------------
 * Classical, non-differentiable "Origin" kernels of OriginUniversal (tools_origin.py:445-804).
 * Build-defined OPSPEC (parity unpinned), see oracle/isp_oracle.py origin_*.  Images are NCHW fp32
 * scaled to 0..255; outputs are clipped and rounded to 8-bit codes; reflect-101 borders.
 * in_scale / out_div: every input sample is multiplied by in_scale first and every output code is
 * multiplied by the fp32 reciprocal of out_div last (how PyTorch divides a GPU tensor by a scalar) - (1,1) for the plugin boundary, which receives x255 images and divides the
 * result itself (tools_origin.py:455,471), (255,255) when the fused pipeline works on [0,1] tensors
 * directly (bit-identical: the same fp32 multiply and divide, minus two passes over the image).
 * out_div < 0 (diagnostic): the clip-and-round is skipped and the unquantised value / |out_div| is stored, so that
 * tests can compare the arithmetic in front of the 8-bit rounding at float tolerance (the median always returns codes).
 * ------------------------------------------------------------------------- */
/* demosaic 'bilinear' (laplacian=0) / 'laplacian' (Malvar-He-Cutler, laplacian=1) - :457-468, :491-502 */
int risp_origin_demosaic(const float *bayer, float *bgr, int laplacian, int N, int H, int W, float in_scale,
                         float out_div, void *stream);
/* spatialnoisereduction 'bilateral' - :686-710.  window (N) odd <= 17, sigmas (N) in 0..255 units */
int risp_origin_bilateral(const float *x, float *y, const int32_t *window, const float *sigma_color,
                          const float *sigma_space, int max_window, int N, int H, int W, float in_scale,
                          float out_div, void *stream);
/* 'median' - :734-751; one odd size <= 17 for the whole batch; works on 8-bit codes */
int risp_origin_median(const float *x, float *y, int size, int N, int H, int W, float in_scale, float out_div,
                       void *stream);
/* 'fastnlm' - :775-797; block_size / search_block (N) odd, decay (N) */
int risp_origin_fastnlm(const float *x, float *y, const int32_t *block_size, const int32_t *search_block,
                        const float *decay, int max_block, int max_search, int N, int H, int W, float in_scale,
                        float out_div, void *stream);
/* globaltonemapping 'reinhard' (mode 0: a=white_point, b=middle_grey), 'crysisengine' (1: a=lum_adapted),
 * 'filmic' (2: a=white_point, b=exposure_bias) - :526-543, :566-581, :604-623; whitebalance
 * 'whiteworld' (3: a=white_point_ratio, stats from risp_channel_stats) - :647-662.
 * a, b: (N) device arrays; scratch: risp_origin_tonemap_scratch_floats(N) floats (per-image constants and the
 * partial sums of Reinhard's log-average luminance, added in a fixed order: deterministic).
 * HW % 4 == 0, and x and y 16-byte aligned (the planes are read and written in 16-byte vectors): anything else is
 * refused before a launch and the message names the pointer. */
size_t risp_origin_tonemap_scratch_floats(int N);
int risp_origin_tonemap(const float *x, float *y, int mode, const float *a, const float *b, const float *stats,
                        float *scratch, int N, int HW, float in_scale, float out_div, void *stream);
/* 'bm3d' (sRGB index 15; the reference has only a proxy net for it) - OPSPEC, restated in float64 in
 * tests/bm3d_reference.py.  Per-image device arrays: sigma (= 2.55 * cff, codes), n1 (4 | 8), cspace (0 orthonormal
 * opponent Y=(R+G+B)/sqrt3 U=(R-B)/sqrt2 V=(R-2G+B)/sqrt6, 1 BT.601 full-range YCbCr without offsets; inverse = the
 * float64 matrix inverse as fp32 constants), wtransform (0 orthonormal DCT-II, 1 orthonormal Haar, full
 * decomposition), radius R (0..9).
 *  1 codes q = floor(clamp(x*in_scale, 0, 255) + 0.5); sigma < 1e-3: the result is q / |out_div| (both output forms).
 *  2 reference blocks n1 x n1 at corners {0, 3, 6, ...} u {H-n1} x the same for W, row-major (no padding).
 *  3 matching on S = B+G+R of the codes: every corner within +-R (clamped to the image) gets D = sum (S_c - S_ref)^2
 *    (int32); kept if D <= 22500 n1^2; ordered by (D, y, x) with the reference forced to rank 0; N2 = the largest
 *    power of two <= min(#kept, 16).  Both filtering steps use this one group.
 *  4 step 1, per colour channel c with sigma_c = sigma * |row_c|: 2D transform of each block, orthonormal Haar along
 *    the group, keep |coef| > 2.7 sigma_c (N_c kept), invert; weight w1 = 1 / sum_c sigma_c^2 max(N_c, 1).
 *  5 aggregation: estimate = sum w K.block / sum w K per pixel and channel, K = outer(kaiser(n1, beta 2)), summed in
 *    (reference index, rank) order - deterministic, no atomics.
 *  6 step 2 on the same groups: pilot P = basic estimate, Z = noisy; W = T(P)^2 / (T(P)^2 + sigma_c^2), estimate
 *    T^-1(W T(Z)), w2 = 1 / sum_c sigma_c^2 max(sum W_c^2, 1) (the floor keeps an all-black group finite); aggregate.
 *  7 inverse colour transform, then the Origin output convention above.
 * The batch runs in chunks of as many images as scratch holds (>= risp_origin_bm3d_scratch_bytes(1, H, W), 256-byte
 * aligned).  groups (nullable): (N, rows, 17) int32 with rows = the grid size for n1 = 4 - count N2, the member
 * corners y*W+x (reference first), -1 padded; rows past an n1 = 8 image's grid are (0, -1, ...).
 * The per-image values are the caller's to validate (functional.origin_denoise refuses bad ones): on the device an
 * n1 other than 4 runs as 8 (as 4 on images smaller than 8), R is clamped to 0..9 - nothing is read or written
 * outside the image, the table and the scratch.  4 <= H, W <= 65535 and 3 H W < 2^31 (anything else is refused, and
 * risp_origin_bm3d_scratch_bytes returns 0 for it). */
size_t risp_origin_bm3d_scratch_bytes(int N, int H, int W);
int risp_origin_bm3d(const float *x, float *y, const float *sigma, const int32_t *n1, const int32_t *cspace,
                     const int32_t *wtransform, const int32_t *radius, int N, int H, int W, float in_scale, float out_div,
                     void *scratch, size_t scratch_bytes, int32_t *groups, void *stream);

/* DemosaicNet (demosaic index 04, tools_origin.py:289-308) - OPSPEC, restated in float64 in tests/demosaicnet_reference.py:
 * Gharbi et al. 2016, Bayer model, depth 15, width 64, in the layout of the public `demosaicnet` package (BayerDemosaick).
 * x (N,1,H,W): an RGGB mosaic in [0,1]; m3 = the masked mosaic, 3 channels (RGB), x at the channel's own CFA sites and 0
 * elsewhere (never materialised: every consumer reads x and the site parity).
 *  1 half resolution (H/2 x W/2): p = pack_mosaic(m3) (2x2 stride-2 conv 3 -> 4, no ReLU); f = relu(conv15(... relu(conv1(p))))
 *    with 3x3 zero-padded convs 4 -> 64, 64 -> 64 (x13), 64 -> 128; filters, masks = f[:, :64], f[:, 64:];
 *    r = residual_predictor(filters * masks) (1x1 64 -> 12).
 *  2 up = upsampler(r): ConvTranspose2d(12, 3, 2, stride 2, groups 3), up[c](2y+dy, 2x+dx) = b[c] + sum_j Wup[4c+j][dy][dx] r[4c+j].
 *  3 full resolution: h = relu(post_conv(cat(m3, up))) (3x3 6 -> 64, zero padding), y = output(h) (1x1 64 -> 3).
 *  4 y (N,3,H,W) fp32 in BGR order, neither clipped nor quantised.
 * The host folds pack_mosaic into conv1 (a selection on the 1-channel mosaic, its bias as border-case planes), the BGR order
 * into the rows of `output` and, for weights trained on GRBG, a mirror along x; the body runs on risp_conv2d*.  Weights here:
 * w_rp (12,64), b_rp (12), w_up (12,2,2), b_up (3), w_post (64,6,3,3) (input channels m3 R G B, up R G B), b_post (64),
 * w_out (3,64) and b_out (3) in OUTPUT order (BGR after the fold).
 * Limits (anything else is refused): 1 <= N <= 65535; H, W even and >= 4; H W 4 < 2^31 (one full-resolution plane below
 * 2^31 bytes; the 64-channel half-resolution tensors are addressed with 64-bit offsets).  up, y, g_up, g_x, add 8-byte
 * aligned.  Deterministic: no atomics, every sum in a fixed order, nothing depends on the batch position.
 *   tail_fwd: filt, mask (N,64,H/2,W/2) post-ReLU halves of conv15 -> up (N,3,H,W); r stays in registers.
 *   tail_bwd: g_up (N,3,H,W) -> the gradients at conv15's pre-activations: g_filt = (W_rp^T g_r) * mask * [filt > 0],
 *             g_mask = (W_rp^T g_r) * filt * [mask > 0], g_r[4c+j](y,x) = sum_{dy,dx} Wup[4c+j][dy][dx] g_up[c](2y+dy, 2x+dx).
 *   head_fwd: (x, up) -> y in one launch (the 64 hidden values of a pixel stay in registers; a 32 x 32 tile plus halo of the
 *             mosaic and the three up planes staged in LDS; fp32).
 *   head_bwd: g_y (N,3,H,W) -> g_up (N,3,H,W) and g_x (N,1,H,W) = add + the direct mosaic term (the m3 channel of each
 *             site); h is recomputed on the tile plus halo and g_h = (W_out^T g_y) * [h > 0] walks LDS 8 hidden channels
 *             at a time.  add (N,1,H,W) is nullable. */
int risp_dmnet_tail_fwd(const float *filt, const float *mask, const float *w_rp, const float *b_rp, const float *w_up,
                        const float *b_up, float *up, int N, int H, int W, void *stream);
int risp_dmnet_tail_bwd(const float *g_up, const float *filt, const float *mask, const float *w_rp, const float *w_up,
                        float *g_filt, float *g_mask, int N, int H, int W, void *stream);
int risp_dmnet_head_fwd(const float *x, const float *up, const float *w_post, const float *b_post, const float *w_out,
                        const float *b_out, float *y, int N, int H, int W, void *stream);
int risp_dmnet_head_bwd(const float *g_y, const float *x, const float *up, const float *w_post, const float *b_post,
                        const float *w_out, const float *add, float *g_up, float *g_x, int N, int H, int W, void *stream);

/* Fused stencil segment (inference): [nearest demosaic ->] bilateral -> element-wise chain in one launch;
 * the BGR halo tile is staged in LDS (straight from the mosaic when from_bayer), every stage output is
 * written ([0,1] domain; the bilateral works on x255 values and returns codes/255 like the reference
 * wrapper, tools_origin.py:690,716).  ops/params/outs as in risp_chain_fwd (no demosaic op). W % 4 == 0.
 * from_bayer with max_window == 3 and a 16-byte aligned mosaic runs without LDS and without a barrier: a thread
 * owns two mosaic quads (2 x 4 pixels) and loads the ring of quads around them itself; same bits either way.
 * Rules (anything else is refused before a launch): max_window odd, 1 .. 17 (1: radius 0, the 8-bit rounding alone);
 * window[n] is clamped to [1, max_window]; 1 <= N <= 65535, H even, W % 4 == 0, H and W > max_window / 2 (one
 * reflection reaches every tap).  0 <= n_ops <= RISP_MAX_CHAIN, ops[k] one of SKIP, WB_MANUAL, GAMMA, GTM_MANUAL,
 * WB_QUADRATIC, GAIN3 in ANY order and any number of times each (every stage has its own parameter block and output);
 * a SKIP stage needs neither params[k] nor outs[k] and may stand anywhere - the last stage that is not a SKIP holds the
 * segment's result.  Alignment: every output 16-byte aligned; the input at any float.  A mosaic with max_window == 3 is
 * read in vectors where it allows them - 16-byte aligned: the quad form, 8-byte: the LDS form with radius 1, otherwise
 * the run-time-radius LDS form, which reads single floats like every other input; the same bits in all three. */
int risp_bilateral_chain_fwd(const float *in, int from_bayer, float *out_demosaic, float *out_bilateral,
                             const int32_t *window, const float *sigma_color, const float *sigma_space,
                             int max_window, int n_ops, const int *ops, const float *const *params,
                             float *const *outs, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------
 * Input side on the device (what the reference's dataset classes do with numpy / cv2 on the host).
 * sel is a device (N,3) int32 array {frame, row, col}; rows / cols even keep the RGGB phase.
 * ------------------------------------------------------------------------- */
/* uint16 RGGB frames (F,H0,W0) -> (N,1,h,w) fp32 = sample / divisor (1023 / 16383:
 * data/oneplus_rggb2obj_dataset.py:201, data/sid_sony_ratio_rggb2bgr_dataset.py:121-134) */
int risp_raw_crop(const uint16_t *frames, float *out, const int32_t *sel, int N, int H0, int W0, int h, int w,
                  float divisor, void *stream);
/* Bayer phase of a sensor, by the mirror that makes its mosaic (even H and W) an RGGB one: cfa = flip_x | flip_y << 1.  The
 * serving entry points below (risp_raw_crop_cfa, risp_serve_u8_cfa, risp_quantise_u8_flip) take it; every other entry point
 * of the library is RGGB. */
#define RISP_CFA_RGGB 0
#define RISP_CFA_GRBG 1 /* mirrored along x */
#define RISP_CFA_GBRG 2 /* mirrored along y */
#define RISP_CFA_BGGR 3 /* mirrored along both */
/* risp_raw_crop for a sensor with a black level and any phase: out (N,1,h,w) is the RGGB window
 * out[n][i][j] = (float)max(s - black_level, 0) / divisor (the subtraction in integers) with
 * s = frames[frame][row + (fy ? h-1-i : i)][col + (fx ? w-1-j : j)], fx = cfa & 1, fy = cfa >> 1.
 * Rules: those of risp_raw_crop; cfa 0 .. 3; 0 <= black_level <= 65535; w even where fx is set and h even where fy is set
 * (row / col even, as for every crop).  black_level 0 and cfa 0 give risp_raw_crop's values. */
int risp_raw_crop_cfa(const uint16_t *frames, float *out, const int32_t *sel, int N, int H0, int W0, int h, int w,
                      float divisor, int black_level, int cfa, void *stream);
/* uint8 HWC BGR ground truth (F,H0,W0,3) -> (N,3,h,w) fp32 / 255 */
int risp_gt_crop(const uint8_t *frames, float *out, const int32_t *sel, int N, int H0, int W0, int h, int w,
                 void *stream);
/* OnePlus "resize by quad" (data/util.py:37-64, oneplus_rggb2obj_dataset.py:109-145): each colour plane of
 * src (H0,W0) is resized to (resized_h/2, W/2) by nearest neighbour and placed pad_top rows down in the
 * zero-filled dst (H,W). */
int risp_resize_rggb(const uint16_t *src, uint16_t *dst, int H0, int W0, int H, int W, int resized_h, int pad_top,
                     void *stream);

/* tensor2bgr + psnr on device (utils/util.py:118-154): truncating uint8 conversion of both images, squared error accumulated
 * in fp64 into sse[0].  sse: risp_sse_uint8_doubles() doubles - sse[1 ..] receive the workgroups' partial sums, added in index
 * order by a finishing launch (no atomics: the same bits on every run). */
size_t risp_sse_uint8_doubles(void);
int risp_sse_uint8(const float *a, const float *b, double *sse, size_t sse_doubles, size_t numel, void *stream);

/* ---------------------------------------------------------------------------
 * SSIM (risp_ssim.hip): get_ssim of the reference (utils/util_path_restore.py:27-44 - scikit-image's compare_ssim with
 * multichannel=True and its defaults): uniform 7 x 7 window, K1 = 0.01, K2 = 0.03, C1 = (K1 L)^2, C2 = (K2 L)^2, sample
 * covariance (49 / 48), S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) averaged over the windows that
 * lie wholly inside the image, then over the channels.  x, y: planar fp32 (N,C,H,W), H, W >= 7, N C H W < 2^31,
 * N C <= 65535.  L: data_range[n] (N floats ON THE DEVICE, no host read) or, data_range == NULL, data_range_scalar.
 * ------------------------------------------------------------------------- */
/* ssim[n], n < N.  quantise != 0: both images first go through tensor2bgr's arithmetic (utils/util.py:130-131,
 * clip(v * 255, 0, 255) truncated, as risp_sse_uint8) and L is in codes (255 for the drivers' metric).  scratch:
 * risp_ssim_scratch_floats(N, C, H, W) floats (one partial sum per workgroup; a finishing launch adds them in index order in
 * fp64: no atomics, the same bits on every run).  Two launches. */
size_t risp_ssim_scratch_floats(int N, int C, int H, int W);
int risp_ssim_fwd(const float *x, const float *y, const float *data_range, float data_range_scalar, int quantise, float *ssim,
                  float *scratch, size_t scratch_floats, int N, int C, int H, int W, void *stream);
/* gx = d (sum_n gs[n] ssim[n]) / dx of the unquantised form (gs: N floats on the device; gx (N,C,H,W), every element
 * written).  One launch that recomputes the window terms from x and y: nothing is kept from the forward call and no
 * scratch is needed.  The target y receives no gradient. */
int risp_ssim_bwd(const float *x, const float *y, const float *data_range, float data_range_scalar, const float *gs, float *gx,
                  int N, int C, int H, int W, void *stream);

/* ---------------------------------------------------------------------------
 * Serving path (risp_serve.hip): 8-bit images on the device.
 * ------------------------------------------------------------------------- */
/* tensor2bgr on the device (utils/util.py:87-94), batched: planar fp32 x (N,C,H,W) -> packed bytes out (N,H,W,C),
 * out = clip(x * 255, 0, 255) truncated, the product in fp32 (the bytes risp_sse_uint8 scores).  C is 1 or 3; any N, H,
 * W >= 1, odd sizes included.  reverse_channels != 0 stores the channels in reverse order (RGB from the library's BGR).
 * x at any float, out at any byte (16-byte / 4-byte aligned buffers with H W % 4 == 0 take the vector form). */
int risp_quantise_u8(const float *x, uint8_t *out, int N, int C, int H, int W, int reverse_channels, void *stream);
/* risp_quantise_u8 of the mirrored image: output pixel (y, x) takes input (fy ? H-1-y : y, fx ? W-1-x : x), fx = flip & 1,
 * fy = flip >> 1 (the RISP_CFA_* bits: it puts the result of an RGGB pipeline run on a mirrored mosaic back in the sensor's
 * orientation).  Rules: those of risp_quantise_u8 - any N, H, W >= 1, C 1 or 3 - and flip 0 .. 3; flip 0 is risp_quantise_u8.
 * (16-byte / 4-byte aligned buffers with W % 4 == 0 take the vector form: a mirrored vector is four pixels of one row.) */
int risp_quantise_u8_flip(const float *x, uint8_t *out, int N, int C, int H, int W, int reverse_channels, int flip,
                          void *stream);
/* A fixed pipeline as an ISP, one launch: raw (N,H,W) uint16 RGGB frames -> out (N,H,W,3) bytes.  Per pixel:
 * (float)sample / divisor (risp_raw_crop's expression), nearest demosaic, the bilateral of risp_bilateral_chain_fwd
 * (x255 domain, 8-bit rounding) when max_window is 1 or 3 - window[n] clamped to [1, max_window]; max_window == 0: no
 * bilateral stage, window / sigma_color / sigma_space are ignored - then the element-wise stages ops[k] with params[k]
 * as in risp_bilateral_chain_fwd, in registers, and the conversion of risp_quantise_u8.  Only the result is stored; its
 * bytes are those of risp_raw_crop -> risp_bilateral_chain_fwd (risp_chain_fwd without a bilateral) -> risp_quantise_u8.
 * No LDS, no barrier: a thread owns a 2 x 4 pixel patch.
 * Rules (anything else is refused before a launch): raw and out not NULL, raw 8-byte and out 4-byte aligned, whole
 * contiguous frames; divisor > 0; max_window 0, 1 or 3; 1 <= N <= 65535, H even and >= 2, W % 4 == 0 and >= 4;
 * 0 <= n_ops <= RISP_MAX_CHAIN, ops[k] one of SKIP, WB_MANUAL, GAMMA, GTM_MANUAL, WB_QUADRATIC, GAIN3 in any order and
 * any number of times each (no DEMOSAIC_NEAREST: the demosaic is implied); every stage but a SKIP needs params[k]. */
int risp_serve_u8(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color,
                  const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params,
                  uint8_t *out, int reverse_channels, int N, int H, int W, void *stream);

/* risp_serve_u8 for a sensor with a black level and any Bayer phase, still one launch and no other pass: raw (N,H,W) is the
 * sensor's mosaic, out (N,H,W,3) the image in the sensor's orientation.  The input expression is
 * (float)(s > black_level ? s - black_level : 0) / divisor, the subtraction in integers (divisor: white level - black level),
 * and the kernel mirrors its addresses (loads at W-1-x / H-1-y, stores at the un-mirrored place) so that its arithmetic is
 * risp_serve_u8's on the RGGB image:
 *     out == unflip(risp_serve_u8(flip(max(raw - black_level, 0)), divisor, ...))   byte for byte,
 * flip mirroring x where cfa & 1 and y where cfa & 2 (RISP_CFA_*).  black_level 0 and cfa 0 give risp_serve_u8's bytes.
 * Rules: those of risp_serve_u8 (H even and W % 4 == 0 make every mirror a phase change), plus cfa 0 .. 3 and
 * 0 <= black_level <= 65535; anything else is refused before a launch and the message names the value. */
int risp_serve_u8_cfa(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color,
                      const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params,
                      uint8_t *out, int reverse_channels, int N, int H, int W, int black_level, int cfa, void *stream);

/* A classical pipeline as an ISP, one launch (risp_serve_classical.hip): raw (N,H,W) uint16 mosaic of the sensor -> out
 * (N,H,W,3) bytes.  Per pixel: (float)max(s - black_level, 0) / divisor (risp_raw_crop_cfa's expression), the demosaic, the
 * stages ops[k] in registers, the conversion of risp_quantise_u8.  Only the result is stored; its bytes are those of
 * risp_raw_crop_cfa -> risp_chain_fwd with DEMOSAIC_NEAREST | risp_origin_demosaic(in_scale 255, out_div 255) -> per stage
 * risp_chain_fwd | risp_origin_tonemap(in_scale 255, out_div 255) -> risp_quantise_u8_flip.
 * demosaic: RISP_DEMOSAIC_NEAREST (the sample as it is), BILINEAR or LAPLACIAN (Malvar-He-Cutler): risp_origin_demosaic's
 * expressions on sample x 255, reflect-101 borders over radius 2, the result rounded to its 8-bit code / 255.
 * ops[k]: SKIP, WB_MANUAL, GAMMA, GTM_MANUAL, WB_QUADRATIC, GAIN3 as in risp_serve_u8, or RISP_OP_TONE_CRYSIS (params (N,1):
 * lum_adapted) / RISP_OP_TONE_FILMIC (params (N,2): white_point, exposure_bias in 1 .. 10): risp_origin_tonemap's curves and
 * 8-bit rounding, their per-image constants formed in the kernel (no prepare launch).  No bilateral here.
 * black_level and cfa as in risp_serve_u8_cfa: the phase is a mirror of addresses, the arithmetic is that of the RGGB image.
 * No LDS, no barrier: a thread owns a 2 x 4 pixel patch and loads its 6 x 8 mosaic neighbourhood itself.
 * Rules (anything else is refused before a launch): raw and out not NULL, raw 8-byte and out 4-byte aligned, whole
 * contiguous frames; divisor > 0; demosaic 0 .. 2; 1 <= N <= 65535, H even and >= 4, W % 4 == 0 and >= 4;
 * 0 <= n_ops <= RISP_MAX_CHAIN, every stage but a SKIP needs params[k]; cfa 0 .. 3; 0 <= black_level <= 65535. */
#define RISP_DEMOSAIC_NEAREST 0
#define RISP_DEMOSAIC_BILINEAR 1
#define RISP_DEMOSAIC_LAPLACIAN 2
int risp_serve_classical_u8(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                            const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W,
                            int black_level, int cfa, void *stream);

/* YUV 4:2:0 (NV12) out of the serving path (risp_nv12.hip, risp_nv12.h).  For an image of H x W pixels, H and W even, the
 * NV12 image is (3H/2, W) bytes, images contiguous: rows 0 .. H-1 are the Y plane, row H + j holds U(j,0) V(j,0) U(j,1)
 * V(j,1) ... for the W/2 chroma sites of quad row j.  With B, G, R the 8-bit codes of a pixel and coef = cy[4], cu[4], cv[4],
 * each row kR, kG, kB, offset:
 *     Y(y,x) = (cy0*R + cy1*G + cy2*B + cy3) >> 8                     per pixel
 *     Rm     = (R00 + R01 + R10 + R11 + 2) >> 2  (Gm, Bm likewise)    per 2 x 2 quad: the rounded mean of the CODES
 *     U(j,i) = (cu0*Rm + cu1*Gm + cu2*Bm + cu3) >> 8,  V(j,i) = (cv0*Rm + cv1*Gm + cv2*Bm + cv3) >> 8
 * chroma sited at the quad centre (JPEG, MPEG-1).  The offsets carry the rounding constant (128) and the plane offset
 * (16 << 8, 128 << 8): every intermediate is a non-negative 32-bit integer, there is no clamp and no signed shift.  A matrix
 * is accepted only if that holds for all codes: per row |k| <= 256, offset + 255 * (sum of positive k) <= 65535 and
 * offset + 255 * (sum of negative k) >= 0; a refusal names the row (cy, cu, cv).  BT.601 full range, the default of the
 * Python side: {77, 150, 29, 128,  -43, -84, 127, 32896,  127, -106, -21, 32896}.
 *
 * risp_bgr8_to_nv12: img (N,H,W,3) packed bytes, B,G,R per pixel or R,G,B with rgb_in != 0 -> nv12 (N,3H/2,W), one launch,
 * 3 bytes read and 1.5 written per pixel.  The end of every serving route that has no fused NV12 store.  With W % 4 == 0 and
 * both buffers 4-byte aligned a thread owns a 2 x 4 patch (three dword loads per row, one Y dword per row and one UV dword
 * stored); otherwise a thread owns one quad and moves bytes.  Rules (anything else is refused before a launch and nothing is
 * written): img, nv12 and coef not NULL, N >= 1, H and W even and >= 2, a valid matrix.  img and nv12 must not overlap. */
int risp_bgr8_to_nv12(const uint8_t *img, uint8_t *nv12, const int32_t coef[12], int rgb_in, int N, int H, int W, void *stream);

/* risp_serve_u8_cfa with the NV12 store: signature, rules, black level and cfa are that entry point's, with the matrix coef
 * in place of reverse_channels and out (N,3H/2,W).  One launch, 2 bytes read and 1.5 written per pixel.  The pixel pipeline
 * is risp_serve_u8_cfa's; from the eight codes of its 2 x 4 patch a thread forms eight Y, two quad means and two UV pairs and
 * stores three dwords instead of six, at the un-mirrored place (with cfa & 1 the Y bytes of a row go to column W-4-px in
 * reverse order and the two quads swap places in the UV dword; with cfa & 2 rows py, py+1 go to H-1-py, H-2-py and the
 * chroma row is (H-2-py)/2).  out == risp_bgr8_to_nv12(risp_serve_u8_cfa(..., reverse_channels 0, ...), coef) byte for
 * byte.  The matrix travels by value with the launch; it is validated before the launch as in risp_bgr8_to_nv12. */
int risp_serve_nv12(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color,
                    const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params,
                    uint8_t *out, const int32_t coef[12], int N, int H, int W, int black_level, int cfa, void *stream);

/* risp_serve_classical_u8 with the NV12 store, as risp_serve_nv12 is to risp_serve_u8_cfa: coef in place of
 * reverse_channels, out (N,3H/2,W), every other argument and rule that entry point's, one launch;
 * out == risp_bgr8_to_nv12(risp_serve_classical_u8(..., reverse_channels 0, ...), coef) byte for byte. */
int risp_serve_classical_nv12(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                              const float *const *params, uint8_t *out, const int32_t coef[12], int N, int H, int W,
                              int black_level, int cfa, void *stream);

/* MIPI-packed RAW10 / RAW12 into the serving path (risp_rawpack.hip, risp_rawpack.h): the layout of CSI-2 receivers, V4L2
 * pRAA / pRCC buffers and DNG.  bits is 10 or 12.  An image is H rows of `stride` bytes, stride >= W * bits / 8, W % 4 == 0;
 * image n starts at byte n * H * stride.  The bytes of a row behind the first W * bits / 8 are padding: any content, never read.
 *     RAW10: pixels 4g .. 4g+3 of a row live in bytes 5g .. 5g+4:   P[4g+k] = (byte[5g+k] << 2) | ((byte[5g+4] >> 2k) & 3), k = 0 .. 3
 *            (pixels 0x3FF, 0x000, 0x155, 0x2AA are the bytes FF 00 55 AA 93)
 *     RAW12: pixels 2g, 2g+1 live in bytes 3g .. 3g+2:              P[2g]   = (byte[3g]   << 4) | (byte[3g+2] & 15)
 *                                                                   P[2g+1] = (byte[3g+1] << 4) | (byte[3g+2] >> 4)
 *            (pixels 0xABC, 0x123 are the bytes AB 12 3C)
 * `packed` may start at any byte and `stride` may have any parity.  No byte outside [packed, packed + N * H * stride) is read,
 * and within a row none behind W * bits / 8.  white_level is not implied by the format.  RAW8, RAW14 and 16-bit containers
 * are not covered.
 *
 * risp_raw_unpack: packed -> out (N,H,W) uint16 contiguous, one sample per word, one launch, bits / 8 bytes read and 2 written
 * per pixel.  The front of every serving route that has no fused packed load.  With packed and stride 4-byte aligned a thread
 * loads the 20 / 24 bytes of 16 pixels as dwords; otherwise (and for a row's last, shorter chunk) it copies 4, 2 and 1 bytes
 * per four pixels.  Rules (anything else is refused before a launch, the message names the value): packed and out not NULL,
 * bits 10 or 12, N and H >= 1, W >= 4 and W % 4 == 0, stride >= W * bits / 8, out 8-byte aligned. */
int risp_raw_unpack(const uint8_t *packed, uint16_t *out, int bits, int N, int H, int W, int stride, void *stream);

/* risp_serve_u8_cfa / risp_serve_nv12 on packed frames, still one launch: raw, bits, stride in place of the uint16 pointer, and
 * coef: NULL stores BGR (N,H,W,3) with reverse_channels, non-NULL stores NV12 (N,3H/2,W) with that matrix (validated as in
 * risp_bgr8_to_nv12; reverse_channels is then not read).  bits / 8 bytes read per pixel.  The same kernel: a thread's four
 * centre pixels are one 5-byte group or two 3-byte groups, the pairs left and right of them half a group or one group, and
 * mirrored along x the group at W-4-x is read and reversed; everything behind the sample is unchanged, so
 *     out == risp_serve_u8_cfa | risp_serve_nv12 (risp_raw_unpack(raw), ...)   byte for byte.
 * Rules: those of risp_serve_u8_cfa (H even, W % 4 == 0, ...) without its alignment rule on raw, plus bits 10 or 12 and
 * stride >= W * bits / 8. */
int risp_serve_packed(const uint8_t *raw, int bits, int stride, float divisor, const int32_t *window, const float *sigma_color,
                      const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params,
                      uint8_t *out, int reverse_channels, const int32_t *coef, int N, int H, int W, int black_level, int cfa,
                      void *stream);

/* risp_serve_classical_u8 / risp_serve_classical_nv12 on packed frames, as risp_serve_packed is to risp_serve_u8_cfa /
 * risp_serve_nv12: raw, bits, stride and coef as there, every other argument and rule risp_serve_classical_u8's (H even and
 * >= 4), one launch; out == risp_serve_classical_u8 | risp_serve_classical_nv12 (risp_raw_unpack(raw), ...) byte for byte. */
int risp_serve_classical_packed(const uint8_t *raw, int bits, int stride, float divisor, int demosaic, int n_ops, const int *ops,
                                const float *const *params, uint8_t *out, int reverse_channels, const int32_t *coef, int N,
                                int H, int W, int black_level, int cfa, void *stream);

/* Lens-shading (vignetting and colour-shading) correction into the serving path (risp_shade.hip, risp_shade.h): a gain per pixel
 * and Bayer plane, interpolated from a coarse mesh - DNG's GainMap, the LSC block of a hardware ISP.  An integer function, fixed
 * to the bit.  A map is gains (GH,GW,4) uint16 contiguous, Q12 (4096 is gain 1.0; every uint16 value is allowed, so a gain is
 * below 16), and cell_log2 = k, 2 <= k <= 8.  Node (i,j) sits at sensor pixel (i << k, j << k); GH == ((H-1) >> k) + 2 and
 * GW == ((W-1) >> k) + 2 exactly: the node below / right of the last pixel exists and no read is conditional.  The plane of
 * pixel (y,x) is c = 2 * (y & 1) + (x & 1), y and x being the sensor's coordinates - those of the frame as stored, before any cfa
 * mirror: the map belongs to the sensor, not to the RGGB view.  With cell = 1 << k, i = y >> k, fy = y & (cell-1), j = x >> k,
 * fx = x & (cell-1), G = gains:
 *     top = (cell - fx) * G[i][j][c]   + fx * G[i][j+1][c]
 *     bot = (cell - fx) * G[i+1][j][c] + fx * G[i+1][j+1][c]
 *     g   = ((cell - fy) * top + fy * bot + (1 << (2k-1))) >> 2k          the Q12 gain of the pixel
 *     s'  = min((max(s - black_level, 0) * g + 2048) >> 12, 65535)        the shaded sample
 * in unsigned 32-bit arithmetic: the largest sums are 2^16 * 65535 + 2^15 and 65535 * 65535 + 2048, below 2^32 and not below
 * 2^31.  The black level leaves inside the definition: s' is a sample with black level 0, and the divisor behind it is
 * white_level - black_level.  There is no clamp at the white level.
 *
 * risp_raw_shade: frames -> out (N,H,W) uint16 contiguous of shaded samples, one launch, bits / 8 bytes read and 2 written per
 * pixel plus the map.  The front of every serving route without a fused shading load.  bits 16: raw is rows of `stride` bytes
 * of uint16 (stride even and >= 2 W, raw 2-byte aligned; image n starts at byte n * H * stride); bits 10 / 12: the packed
 * layouts above with their rules - the launch decodes and shades, risp_raw_unpack is not needed.  Rules (anything else is
 * refused before a launch, the message names the value): no NULL, N and H >= 1, W >= 4 and W % 4 == 0, the rules of the map,
 * gains and out 8-byte aligned, black_level 0 .. 65535. */
int risp_raw_shade(const void *raw, int bits, int stride, uint16_t *out, const uint16_t *gains, int cell_log2, int GH, int GW,
                   int black_level, int N, int H, int W, void *stream);

/* risp_serve_classical_u8 / risp_serve_classical_nv12 with the shading inside the load, still one launch: coef NULL stores BGR
 * (N,H,W,3) with reverse_channels, non-NULL stores NV12 (N,3H/2,W) with that matrix, as in risp_serve_classical_packed; divisor
 * is white_level - black_level.  The float that enters the demosaic is (float)s' / divisor; nothing behind the sample changes, so
 *     out == risp_serve_classical_u8 | risp_serve_classical_nv12 (risp_raw_shade(raw, black_level), divisor, ..., black_level 0, cfa)
 * byte for byte.  uint16 frames only.  Rules: those of risp_serve_classical_u8 plus the rules of the map. */
int risp_serve_classical_shaded(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                const float *const *params, uint8_t *out, int reverse_channels, const int32_t *coef,
                                const uint16_t *gains, int cell_log2, int GH, int GW, int N, int H, int W, int black_level,
                                int cfa, void *stream);

/* Defective-pixel correction (DPC) into the serving path (risp_defect.hip, risp_defect.h): hot, dead and factory-listed pixels
 * replaced from their same-colour neighbours, in front of shading and demosaic - DNG's FixBadPixelsConstant / FixBadPixelsList, the
 * DPC block of a hardware ISP.  An integer function of the frame, fixed to the bit (tests/defect_reference.py restates it).
 * S(y,x) is the decoded raw sample of the frame as stored - uint16, or RAW10 / RAW12 as above -, before the black level and whatever
 * cfa says.  An index outside the frame reflects without repeating the edge, i -> -i and i -> 2 (n-1) - i, which keeps the Bayer
 * colour: parity is preserved for every n.  H >= 3, W >= 4, W % 4 == 0.  The neighbour pairs of pixel p = S(y,x), in this order:
 *     H  S(y,x-2),   S(y,x+2)          V  S(y-2,x),   S(y+2,x)
 *     D  S(y-2,x-2), S(y+2,x+2)        A  S(y-2,x+2), S(y+2,x-2)
 *     mx, mn = the maximum and the minimum of the eight neighbours;   T(v) = threshold + ((v * slope) >> 8)
 *     hot     p > mx + T(mx)
 *     dead    p + T(mn) < mn
 *     listed  bit (x & 31) of word (x >> 5) of row y of the defect map is set
 * A pixel that is hot, dead or listed becomes (a + b + 1) >> 1 of the pair (a, b) with the smallest |a - b|; on a tie the first
 * pair in the order H, V, D, A wins.  Every other pixel passes through.  Neighbours are always the input's, never corrected
 * output: the result is a pure function of the frame.  All arithmetic is unsigned 32-bit.  Nothing wraps there, but mx + T(mx),
 * p + T(mn) and a + b + 1 pass 2^16, so a form that keeps them in packed 16-bit lanes is wrong.
 * threshold: 0 .. 65535 in raw codes, or -1 for no dynamic test (then slope is not used); slope: 0 .. 255, Q8 - photon noise grows
 * with the signal.  defects: (H, (W + 31) / 32) uint32 words, contiguous, 4-byte aligned, one map for all N frames, bits at x >= W
 * ignored; NULL for no map.  One of the two must be on.  Not covered: green's nearer diagonal neighbours, clusters of adjacent
 * defects (a defective neighbour enters as it is), thresholds per Bayer plane.
 *
 * risp_raw_defect: frames -> out (N,H,W) uint16 contiguous, one launch, bits / 8 bytes read and 2 written per pixel plus the maps.
 * raw, bits and stride as in risp_raw_shade: uint16 rows (2-byte aligned, wider loads when raw and stride are 8-byte aligned) or
 * packed rows from any byte, decoded on the way.  gains NULL: out holds the corrected raw codes, black level kept, and cell_log2,
 * GH, GW and black_level must be 0.  gains not NULL: each corrected sample is shaded exactly as risp_raw_shade shades it,
 *     out == risp_raw_shade(risp_raw_defect(raw, ..., gains NULL), gains, ..., black_level)   word for word,
 * with the rules of the map.  out must not overlap raw: a thread reads rows other threads write.  Rules (anything else is
 * refused before a launch, the message names the value): raw and out not NULL, N >= 1, H >= 3, W >= 4 and W % 4 == 0, the stride
 * rules of the format, threshold -1 .. 65535, slope 0 .. 255, threshold >= 0 or defects, out 8-byte aligned. */
int risp_raw_defect(const void *raw, int bits, int stride, uint16_t *out, int threshold, int slope, const uint32_t *defects,
                    const uint16_t *gains, int cell_log2, int GH, int GW, int black_level, int N, int H, int W, void *stream);

/* Temporal noise reduction (TNR / 3DNR) into the serving path (risp_temporal.hip, risp_temporal.h): the recursive raw-domain filter
 * of a video ISP, behind defect correction and lens shading and in front of the demosaic.  The one serving block with state across
 * calls.  An integer function of the current frame and the state, fixed to the bit (tests/temporal_reference.py restates it in
 * numpy int64).
 * c is the current frame and p the state - the previous filtered frame -, both (H,W) uint16 in the sample domain the route
 * demosaics: raw codes with pedestal black_level, or shaded samples with black level 0 behind a shading.  The window is the full
 * 5 x 5 around (y,x), all colours - symmetric, so cfa does not enter.  An index outside the frame reflects without repeating the
 * edge (-1 -> 1, -2 -> 2, H -> H-2, H+1 -> H-3), as in the defect correction.  H >= 3, W >= 4, W % 4 == 0.
 *     A  = sum over the window of (c - p)                      signed, |A| <= 25 * 65535
 *     B  = sum over the window of p
 *     Bs = max(B - 25 * black_level, 0)
 *     lo = 25 * threshold + ((Bs * slope) >> 8)
 *     e  = min(max(|A| - lo, 0), 65535)
 *     k  = min(strength + ((e * ramp) >> 8), 256)
 *     out(y,x) = (p(y,x) * (256 - k) + c(y,x) * k + 128) >> 8
 * strength: 0 .. 256, Q8, the share of the new frame where nothing moves - 256 is the identity, 0 freezes; threshold: 0 .. 65535,
 * in codes of mean difference; slope: 0 .. 255, Q8, the part of the threshold that grows with the signal; ramp: 0 .. 65535, Q8 per
 * code of summed excess.  Every intermediate fits unsigned 32 bits: Bs * slope < 4.2e8, e * ramp <= 65535^2, and the blend stays
 * below 2^24 + 128.  With k == 256, out == c exactly.  The new state is out.  Neighbours are always the previous state's and the
 * current frame's: a launch never reads a state value that it wrote itself.
 *
 * risp_raw_temporal: cur, state, out (N,H,W) uint16 contiguous.  ONE launch reads cur and state and writes out (6 bytes per pixel),
 * then ONE device-to-device copy of out into state follows on the same stream (4 more): the state cannot be written in place -
 * other workgroups still read its halo - and two buffers alternated by the host would bake one direction into a captured graph.
 * prime != 0: state is not read, out = cur, and the copy makes state = cur (two copies, no launch).  cur and state 2-byte aligned
 * (wider loads when both are 8-byte aligned), out 8-byte aligned.  out may overlap neither cur nor state.  Rules (anything else
 * is refused before anything is issued, the message names the value): no NULL, N >= 1, H >= 3, W >= 4 and W % 4 == 0,
 * strength 0 .. 256, threshold 0 .. 65535, slope 0 .. 255, ramp 0 .. 65535, black_level 0 .. 65535, the alignments, no overlap of
 * out.  Not covered: motion compensation, a per-plane or per-gain noise model, the filter fused into the defect or shade launch or
 * into a route's own launch, a state updated without the copy, a separate luma / chroma strength, a fix for the recursion stalling
 * at strength < 128 from rounding ((p * (256 - k) + c * k + 128) >> 8 == p once |c - p| * k < 128). */
int risp_raw_temporal(const uint16_t *cur, uint16_t *state, uint16_t *out, int prime, int strength, int threshold, int slope,
                      int ramp, int black_level, int N, int H, int W, void *stream);

/* 3A statistics of the sensor frame (risp_stats.hip): the statistics block of a hardware ISP - per-zone colour sums for
 * auto-white-balance, histograms for auto-exposure, a focus measure for autofocus -, taken on the linear samples the route
 * demosaics.  Counts and sums of integers, fixed to the bit and without a summation order (tests/stats_reference.py restates
 * them in numpy int64).
 * s(y,x) = max(S(y,x) - black_level, 0), S the decoded sample of the frame as stored - uint16, or RAW10 / RAW12 as above.
 * Coordinates are those of the frame as stored, whatever cfa says; the plane of a pixel is c = 2 * (y & 1) + (x & 1).
 * A specification is (zone_h, zone_w, bins, hist_shift, lo, hi).  ZH = ceil(H / zone_h), ZW = ceil(W / zone_w); pixel (y,x)
 * belongs to zone (y / zone_h, x / zone_w); the last row and column of zones may be partial.  For each image, zone and plane:
 *     count  the number of the zone's samples of that plane with lo <= s <= hi
 *     sum    the sum of those samples
 *     sharp  the sum of |2 s(y,x) - s(y,x-2) - s(y,x+2)| over the zone's pixels of that plane with 2 <= x < W - 2, whatever lo
 *            and hi are: a pixel without both neighbours inside the frame adds nothing (no reflection); a neighbour may lie
 *            in the next zone
 * and for each image and plane   hist[min(s >> hist_shift, bins - 1)] += 1   over every sample of the frame.
 *
 * risp_raw_stats: frames -> zones (N,ZH,ZW,4,3) int64 holding [sum, count, sharp] and hist (N,4,bins) int32, both contiguous
 * and both overwritten: they are zeroed on the stream (one memset where hist lies right behind zones, else two), then ONE launch
 * reads bits / 8 bytes per pixel.  The values pass 2^32 on real frames (131072 samples of 65535 already do), which is why zones
 * is 64-bit; a workgroup's partials are 32-bit and bounded by its tile (risp_stats.hip).  raw, bits and stride as in
 * risp_raw_shade: uint16 rows (2-byte aligned, wider loads when raw and stride are 8-byte aligned) or packed rows from any byte,
 * decoded on the way.  Rules (anything else is refused before anything is issued, the message names the value): no NULL,
 * N >= 1, H even, W >= 4 and W % 4 == 0, the stride rules of the format, black_level 0 .. 65535, zone_h even and >= 2,
 * zone_w >= 4 and zone_w % 4 == 0, ZH * ZW <= 65536, bins 1 .. 1024, hist_shift 0 .. 16, 0 <= lo <= hi <= 65535,
 * H * W / 4 < 2^31, zones 8-byte and hist 4-byte aligned.  Not covered: statistics gathered inside another launch, vertical or
 * IIR focus filters, statistics behind the demosaic, per-zone histograms. */
int risp_raw_stats(const void *raw, int bits, int stride, int black_level, long long *zones, int *hist, int zone_h, int zone_w,
                   int bins, int hist_shift, int lo, int hi, int N, int H, int W, void *stream);

/* Auto white balance and auto exposure on the device (risp_control.hip): the 3A controller of a capture loop, the block that reads
 * the statistics above and sets the next frame's gains.  Its output is a lens-shading map - a Q12 gain per Bayer plane, applied
 * in front of everything (risp_raw_shade and every fused shading load) -, and the statistics are taken behind the shading, so
 * rewriting the map from the statistics of frame t closes the loop for frame t+1.  An integer function of zones, hist and the
 * state, fixed to the bit (tests/control_reference.py restates it in numpy int64).
 *
 * Inputs.  zones (N,ZH,ZW,4,3) int64 [sum, count, sharp] and hist (N,4,bins) int32 as risp_raw_stats writes them for N frames of
 * H x W with (zone_h, zone_w, bins, hist_shift); cfa = k, a RISP_CFA_* code: colour q of (r, gr, gb, b) lives in plane q ^ k.
 * The state (e, wr, wb): Q12 unsigned, at most 65535 - the exposure gain and the red and blue white-balance gains; green is
 * 4096.  A control specification is RISP_CONTROL_SPEC_INTS integers, in this order, ranges in brackets:
 *     fill [0..256]   y_lo <= y_hi [0..65535]   rg_lo <= rg_hi, bg_lo <= bg_hi [0..4095, Q8 ratios]   min_share [0..256]
 *     wb_dead [0..4095]   wb_speed [0..256]   wb_min <= wb_max [256..65535]
 *     pct [1..65536]   target [1..65535]   ceil [1..65535]   ae_dead [0..4095]   ae_speed [0..256]   e_min <= e_max [256..65535]
 * The N images of a call are pooled: a call has one state and one gain map.
 *
 * White balance, a grey-candidate gray world over the zones.  For image n and zone (zy,zx): rows = min(zone_h, H - zy * zone_h),
 * cols = min(zone_w, W - zx * zone_w), area = (rows / 2) * (cols / 2) - by the rules of risp_raw_stats every plane of the zone has
 * exactly area samples.
 *     filled     for all four planes  count >= 1  and  count * 256 >= fill * area                           (64-bit)
 *     m          per plane (sum + (count >> 1)) / count, an unsigned 64-bit division; at most 65535 (a quotient above, which
 *                no statistics of risp_raw_stats give, counts as 65535)
 *     mr = m[r]     mg = (m[gr] + m[gb] + 1) >> 1     mb = m[b]
 *     candidate  filled  and  y_lo <= mg <= y_hi  and  rg_lo * mg <= 256 * mr <= rg_hi * mg  and  bg_lo * mg <= 256 * mb <= bg_hi * mg
 *                (unsigned 32-bit: the largest product is 4095 * 65535 < 2^28)
 *     over all candidates   AR += mr   AG += mg   AB += mb   K += 1                                          (64-bit)
 *     solved     K >= 1  and  K * 256 >= min_share * N * ZH * ZW  and  AR > 0  and  AB > 0
 *     solved:    cr = clamp((AG << 12) / AR, 1024, 16384), cb likewise from AB (64-bit);
 *                wr' = damp(wr, cr, wb_dead, wb_speed, wb_min, wb_max), wb' likewise;   otherwise wr' = wr and wb' = wb.
 * Exposure, from the green histograms.
 *     Hg[b] = sum over n of hist[n][gr][b] + hist[n][gb][b]   (64-bit)        T = sum of Hg;   T == 0: e' = e, M = P = 0
 *     v(b)  = min((b << hist_shift) + ((1 << hist_shift) >> 1), 65535)        the bin's centre
 *     M     = (sum of Hg[b] * v(b) + (T >> 1)) / T                            the mean green level
 *     b*    = the smallest b with cum(b) * 65536 >= T * pct,  cum(b) = Hg[0] + .. + Hg[b]
 *     P     = min(((b* + 1) << hist_shift) - 1, 65535)                        the upper edge of that bin
 *     corr  = clamp((target << 12) / max(M, 1), 1024, 16384)
 *     if P * corr > (ceil << 12)   highlight protection takes over:   corr = clamp((ceil << 12) / max(P, 1), 1024, 16384)
 *     e'    = damp(e, corr, ae_dead, ae_speed, e_min, e_max)
 * damp(cur, corr, dead, speed, lo, hi):  |corr - 4096| <= dead makes corr 4096;  step = 4096 + (((corr - 4096) * speed) >> 8), a
 * signed 32-bit arithmetic shift (floor), step in 1024 .. 16384;  the result is clamp((cur * step + 2048) >> 12, lo, hi), with
 * cur * step < 2^30.  Speed 0 switches that half of the controller off.
 * Gains and the map.  g[p] = min((e' * w + 2048) >> 12, 65535) for plane p, w = wr' where p ^ k is r, wb' where it is b, 4096 on
 * the two greens (unsigned 32-bit);  out[i][j][p] = min((base[i][j][p] * g[p] + 2048) >> 12, 65535) for a base map (GH,GW,4)
 * uint16 (unsigned 32-bit: 65535 * 65535 + 2048 < 2^32);  without a base map the base is 4096 everywhere and out == g[p].
 * Sizes.  N * ZH * ZW <= 2^24 and N * H * W / 2 < 2^40, so that every sum fits: AR, AG, AB <= 2^24 * 65535 < 2^40 and
 * AG << 12 < 2^52;  T < 2^40, sum of Hg * v < 2^56, cum * 65536 and T * pct <= 2^56;  count * 256 and fill * area < 2^48.
 *
 * The state is RISP_CONTROL_STATE_INTS = 16 contiguous int32 on the device:  [0] e  [1] wr  [2] wb  [3] updates so far, mod 2^31
 * [4] M  [5] P  [6] min(K, 2^31 - 1)  [7] flags: bit 0 white balance solved, bit 1 T > 0, bit 2 the ceiling took over
 * [8..11] g[0..3]  [12..15] 0.  The host may read it whenever it likes; nothing makes it.
 *
 * risp_control_solve: ONE launch of 256-thread workgroups, one per 256 zones, at least 1 and at most 1024; zones and histogram
 * words are walked grid-stride.  A thread per zone does the four divisions and the candidate test; wave shuffles, then LDS,
 * reduce AR, AG, AB, K per workgroup, the green histogram words go into a copy of Hg in LDS.  scratch is 5 + bins uint64
 * [ticket, AR, AG, AB, K, Hg[bins]], zeroed once by the caller: a workgroup adds its non-zero partials with 64-bit agent-scope
 * atomics and then draws a ticket; the workgroup that draws the last one takes every accumulator with an atomic exchange against
 * 0 - which leaves scratch zero for the next launch or replay -, solves, writes the 16 state words and resets the ticket.  No
 * workgroup waits or polls.  spec is a HOST array, read before the launch.  Rules (anything else is refused before anything is
 * issued, the message names the value): no NULL, the specification's ranges, N >= 1, H even, W >= 4 and W % 4 == 0, zone_h even
 * and >= 2, zone_w >= 4 and zone_w % 4 == 0, ZH == ceil(H / zone_h), ZW == ceil(W / zone_w), the two sizes above, bins 1 .. 1024,
 * hist_shift 0 .. 16, cfa 0 .. 3, zones and scratch 8-byte, hist and state 4-byte aligned.
 *
 * risp_gain_map: one streaming launch, a thread per node: out (GH,GW,4) uint16 from base (NULL: 4096 everywhere) and the state's
 * words 8 .. 11, 8 bytes loaded and 8 stored per node.  Rules: state and out not NULL, GH and GW >= 2, GH * GW <= 2^30, base
 * and out 8-byte and state 4-byte aligned, out may not overlap base.
 * Not covered: metering weights per zone, a per-image gain map, exposure time or analogue gain handed to a sensor driver, flicker
 * and scene-change detection, a colour-temperature prior or locus, the gains folded into an existing map without the second
 * launch, statistics gathered in the shade launch. */
#define RISP_CONTROL_SPEC_INTS 19
#define RISP_CONTROL_STATE_INTS 16
int risp_control_solve(const long long *zones, const int *hist, int *state, unsigned long long *scratch, const int *spec, int N,
                       int ZH, int ZW, int H, int W, int zone_h, int zone_w, int bins, int hist_shift, int cfa, void *stream);
int risp_gain_map(const uint16_t *base, const int *state, uint16_t *out, int GH, int GW, void *stream);

/* A scaled, cropped output at the end of the serving path (risp_resize.hip): the scaler / crop block behind an ISP's colour
 * pipeline.  Packed 8-bit images are resampled separably, antialiased on reduction, with an integer tap table per axis - the
 * design of Pillow's ImagingResample, made reproducible to the bit: Q14 weights, every row of weights sums to exactly 16384, and
 * only IEEE basic operations (+ - * /, comparisons, truncation) build the table, so every machine builds the same integers
 * (tests/resize_reference.py restates all of it in numpy; functional.resample_taps builds the tables on the host).
 *
 * Tap table of one axis.  S is the length of the source window, o its offset in the image, D the output length.  The kernel f
 * has radius r:
 *     box       f(x) = 1 for -0.5 < x <= 0.5, else 0                                  r = 0.5
 *     triangle  f(x) = 1 - |x| for |x| < 1, else 0                                    r = 1
 *     bicubic   Keys, a = -0.5, in Horner form as Pillow's bicubic_filter, t = |x|:
 *               (((a + 2) t - (a + 3)) t) t + 1 for t < 1,  (((t - 5) t + 8) t - 4) a for t < 2, else 0        r = 2
 * All in float64:  scale = S / D,  fs = max(scale, 1),  support = r * fs;  for output index i:  c = (i + 0.5) * scale,
 *     lo = max(int(c - support + 0.5), 0),  hi = min(int(c + support + 0.5), S)        (int truncates)
 *     w_k = f((k + lo - c + 0.5) / fs)  for k < hi - lo;   s = the sum of the w_k, left to right
 *     q_k = floor(w_k / s * 16384 + 0.5);  the residue 16384 - sum(q) is added to the largest q_k (the first on a tie)
 * Zero taps at either end are trimmed (lo moves with them).  T is the longest row.  start_i = min(lo_i, S - T), the row is
 * written at column lo_i - start_i of a zero row of T int16, and then start_i += o.  T <= S always and o <= start_i,
 * start_i + T <= o + S: the window enters only through o, so the result equals cropping first.  Starts never decrease with box
 * and triangle and on every reduction; a bicubic enlargement trims the exact zeros at |x| = 1, 2 of an output that falls on a
 * sample, and that row's start lies one past its neighbour's.
 *
 * Pixel.  Signed 32-bit arithmetic, >> the arithmetic shift (floor); with T <= 32 and int16 weights no sum reaches 2^31.
 *     h(y,j,c)   = clamp((sum_k wx[j][k] * img(y, xs[j]+k, c) + 8192) >> 14, 0, 255)      horizontal first, rounded to a code
 *     out(i,j,c) = clamp((sum_k wy[i][k] * h(ys[i]+k, j, c)   + 8192) >> 14, 0, 255)
 * per channel, so the channel order does not matter.  NV12 out is the integer function above of out, unchanged.
 *
 * risp_bgr8_resize: img (N,H,W,3) -> out (N,OH,OW,3), or with coef (twelve integers as in risp_bgr8_to_nv12, validated
 * likewise; rgb_in as there) -> out (N,3*OH/2,OW) NV12.  One launch, no host synchronisation.  xstart (OW) / ystart (OH) int32
 * and xweight (OW x tx) / yweight (OH x ty) int16 are DEVICE tables as above, tx and ty their T.  A workgroup owns
 * RISP_RESIZE_TILE_W output columns x tile_rows output rows: it resamples the source rows its tile needs horizontally into LDS
 * as bytes, then runs the vertical sums from there.  The rows a tile needs depend on ystart, which this side cannot read: the
 * caller passes tile_rows and span, the largest over all tiles of (largest ystart of its rows) + ty - (their smallest); a span
 * whose rows do not fit RISP_RESIZE_LDS_BYTES is refused (take fewer tile_rows).  Inside the kernel every start is
 * clamped into 0 .. W-1 (H-1) as it is loaded, every source index start + k into the image again, and every LDS row into the
 * span: a wrong table gives wrong bytes - those of the clamped table -, never an access outside img.  No alignment
 * is asked of img or of a BGR out - a packed row starts at any byte.  Rules (anything else is refused before the launch, the
 * message names the value): no NULL pointer but coef, 1 <= N <= 65535, H, W, OH, OW in 1 .. 2^24, 1 <= tx <= min(W,
 * RISP_RESIZE_MAX_TAPS) and ty likewise with H, 1 <= tile_rows <= 64, span >= 1, out not overlapping img; for NV12 OH, OW and
 * tile_rows even and out 4-byte aligned.  functional.resample_taps refuses a geometry as soon as one support window hi - lo
 * passes 32 samples, before trimming - reductions beyond 32:1 (box), 16:1 (triangle), 8:1 (bicubic).  Not covered: Lanczos
 * (needs sin), such reductions, chroma-aware scaling, rotation. */
#define RISP_RESIZE_MAX_TAPS 32
#define RISP_RESIZE_TILE_W 64
#define RISP_RESIZE_LDS_BYTES 65536
int risp_bgr8_resize(const uint8_t *img, uint8_t *out, const int32_t *xstart, const int16_t *xweight, int tx, const int32_t *ystart,
                     const int16_t *yweight, int ty, int tile_rows, int span, const int32_t *coef, int rgb_in, int N, int H, int W,
                     int OH, int OW, void *stream);

/* A geometry-corrected output of the serving path (risp_warp.hip): the LDC / GDC / dewarp block of an ISP - lens-distortion
 * correction, rotation and flips, keystone, the per-frame shift and rotation of electronic stabilisation.  Packed 8-bit images
 * are resampled through a mesh of source coordinates; an integer function, fixed to the bit (tests/warp_reference.py restates
 * all of it in numpy int64; functional.warp_mesh / warp_homography / warp_radial build meshes on the host).
 *
 * Source: img, packed 8-bit (N,H,W,3); every channel is treated alike, so the channel order does not matter.  Output (N,WH,WW,3).
 *
 * Mesh: (MH,MW,2) int32, contiguous, with cell_log2 = k, 2 <= k <= 8, cell = 1 << k.  Node (i,j) sits at output pixel
 * (i << k, j << k); mesh[i][j][0] is the source y of that pixel, mesh[i][j][1] its source x, in Q8: 256 is one pixel, coordinate 0
 * the centre of source pixel 0, signed, possibly outside the image.  MH == ((WH-1) >> k) + 2 and MW == ((WW-1) >> k) + 2
 * exactly - the rule of the shading map: the node below and right of the last pixel exists, so no read is conditional.  One
 * mesh serves every image of the call.
 *
 * Per-pixel coordinate: signed 64-bit arithmetic.  For output pixel (y,x): i = y >> k, fy = y & (cell-1), j = x >> k,
 * fx = x & (cell-1); for component c with S = H for c = 0 and S = W for c = 1
 *     top = (cell - fx) * M[i][j][c]   + fx * M[i][j+1][c]
 *     bot = (cell - fx) * M[i+1][j][c] + fx * M[i+1][j+1][c]
 *     u_c = ((cell - fy) * top + fy * bot + (1 << (2k-1))) >> 2k          >> the arithmetic shift (floor)
 *     u_c = clamp(u_c, 0, (S-1) << 8)                                      the replicate border
 * Every int32 mesh is a defined input; the sums stay below 2^48.  The clamp comes after the interpolation: a node outside the
 * image - the extra node of a flip - enters unclamped.
 *
 * kernel 0, bilinear: y0 = uy >> 8, ty = uy & 255, y1 = min(y0+1, H-1), and x0, tx, x1 likewise with W; per channel
 *     out = ((256-ty) * ((256-tx)*p[y0][x0] + tx*p[y0][x1]) + ty * ((256-tx)*p[y1][x0] + tx*p[y1][x1]) + 32768) >> 16
 * exact, every sum below 2^24, no clamp needed.
 *
 * kernel 1, bicubic: Catmull-Rom (a = -1/2) with Q11 weights from integers only.  For the phase f in 0 .. 255
 *     n0 = -f^3 + 512 f^2 - 65536 f      n1 = 3 f^3 - 1280 f^2 + 2^25
 *     n2 = -3 f^3 + 1024 f^2 + 65536 f   n3 = f^3 - 256 f^2                (they sum to 2^25; each |n| < 2^31)
 *     q_t = (n_t + 8192) >> 14,  then q[first index of the largest q] += 2048 - (q0+q1+q2+q3)
 * so every row sums to 2048; row 0 is (0, 2048, 0, 0), row 128 (-128, 1152, 1152, -128).  Taps are rows y0-1 .. y0+2 and
 * columns x0-1 .. x0+2, every index clamped into the image:
 *     h_r = sum_c q[tx][c] * p[row r][col c];   v = sum_r q[ty][r] * h_r;   out = clamp((v + (1 << 21)) >> 22, 0, 255)
 * with no intermediate rounding; |v| + 2^21 <= 1 370 357 760 + 2^21 < 2^31 (Q12 would overflow, Q11 does not).
 *
 * Consequences (tests/test_warp_reference_cpu.py): the identity mesh returns img; the mesh of (H-1-y, W-1-x) returns img flipped
 * on both axes; the mesh of (x, y) with size (W,H) the transpose; an affine map's per-pixel coordinate lies within 1 Q8 unit of
 * 256 times the exact value (1/2 from rounding the nodes, 1/2 from the final rounding).
 *
 * risp_bgr8_warp: one launch, no host synchronisation, capturable.  kernel 0 / 1 as above.  A workgroup owns
 * RISP_WARP_TILE_W x RISP_WARP_TILE_H output pixels: it evaluates their coordinates, reduces them to the tile's source
 * bounding box - taps and border clamp included - and, with stage = 1, loads that box into LDS with aligned dword loads and
 * samples from there where the box fits RISP_WARP_LDS_BYTES (beside 5136 bytes of weights and output tile); a tile whose box
 * does not fit - a strong reduction, a twisted cell, a meaningless mesh - samples global memory, decided per tile inside the
 * launch.  stage = 0 makes every tile sample global memory; both forms are the same integer function.  The bicubic weights are
 * computed in the kernel.  No alignment is asked of img or out - a packed row starts at any byte -, and no byte outside img,
 * mesh or out is read or written whatever the mesh holds, the last partial dword of img included.  Rules (anything else is
 * refused before the launch, the message names the value): no NULL pointer, 1 <= N <= 65535, H, W, WH, WW in 1 .. 2^23 (a Q8
 * coordinate fits int32), 2 <= cell_log2 <= 8, MH and MW exactly as defined, kernel and stage in {0, 1}, out not overlapping
 * img, at most 65535 row tiles, mesh 8-byte aligned.  Not covered: a fill colour outside the image, antialiasing of reductions
 * beyond about 2:1 (resize behind the warp: out_size), chroma-aware warping, a per-image mesh, meshes that are not bilinear
 * patches. */
#define RISP_WARP_TILE_W 64
#define RISP_WARP_TILE_H 16
#define RISP_WARP_LDS_BYTES 65536
int risp_bgr8_warp(const uint8_t *img, uint8_t *out, const int32_t *mesh, int cell_log2, int MH, int MW, int kernel, int stage,
                   int N, int H, int W, int WH, int WW, void *stream);

/* Output sharpening of the serving path (risp_sharpen.hip): the edge-enhancement (EE) block between the scaler and the YUV
 * output of an ISP - an unsharp mask of luma with coring and a limit.  An integer function of packed 8-bit images, fixed to the
 * bit (tests/sharpen_reference.py restates all of it in numpy int64).
 *
 * Source: img, packed 8-bit (N,H,W,3), B,G,R per pixel or R,G,B with rgb_in != 0.  Parameters: radius 1 or 2, amount
 * 0 .. RISP_SHARPEN_MAX_AMOUNT (Q8: 256 is a gain of 1.0), threshold 0 .. 255 and limit 0 .. 255 (codes).  All arithmetic is
 * unsigned or signed 32-bit and nothing can overflow: 65280 * 4095 + 32768 < 2^32.
 *
 *     luma      L = (77 R + 150 G + 29 B + 128) >> 8                    0 .. 255; the weights do not depend on any YUV matrix
 *     blur      S = sum over the (2 radius + 1)^2 window of w * L        Q8, no intermediate rounding
 *               radius 2: w = [1 4 6 4 1] (x) [1 4 6 4 1]; radius 1: w = 16 * ([1 2 1] (x) [1 2 1]); both sum to 256
 *               window indices are clamped to 0 .. H-1 and 0 .. W-1 (replicate border, the warp's rule): every size from
 *               1 x 1 is defined
 *     detail    D = 256 L - S                                            signed, exact, |D| <= 65280
 *     coring    A = max(|D| - 256 threshold, 0)                          soft: the threshold is subtracted, not only compared
 *     gain      E = min((A * amount + 32768) >> 16, limit)               the limit follows the gain
 *     output    c' = min(max(c + sign(D) * E, 0), 255)                   the same E for B, G and R
 *
 * The enhancement is of luma only: chroma differences are kept until a channel clips.  With amount == 0 or limit == 0 the
 * image passes unchanged (still one launch).
 *
 * risp_bgr8_sharpen: one launch for all N images, no host synchronisation, capturable.  With coef == NULL out is (N,H,W,3)
 * packed bytes in the channel order of img; with coef (twelve integers as in risp_bgr8_to_nv12, validated alike; H and W even)
 * out is NV12 (N,3H/2,W) of the sharpened codes, byte for byte
 * risp_bgr8_to_nv12(risp_bgr8_sharpen(.., NULL, ..), coef, rgb_in).  A workgroup owns RISP_SHARPEN_TILE_W x
 * RISP_SHARPEN_TILE_H pixels and stages their source box, widened by the radius and clamped into the image, in LDS.  No
 * alignment is asked of img or out - a packed row starts at any byte -, and no byte outside the two images is read or written
 * for any H, W >= 1, the last partial dword of img included.  Rules (anything else is refused before the launch, the message
 * names the value): no NULL img or out, 1 <= N <= 65535, H and W in 1 .. 2^24, at most 65535 row tiles, the parameter ranges
 * above, out not overlapping img.  Not covered: overshoot control by local extremes, separate gains for dark and bright halos,
 * a noise-adaptive threshold, sharpening fused into the resize or warp launch, chroma noise reduction. */
#define RISP_SHARPEN_TILE_W 64
#define RISP_SHARPEN_TILE_H 16
#define RISP_SHARPEN_MAX_AMOUNT 4095
int risp_bgr8_sharpen(const uint8_t *img, uint8_t *out, const int32_t *coef /* 12 integers or NULL */, int rgb_in, int radius,
                      int amount, int threshold, int limit, int N, int H, int W, void *stream);

/* Scene-adaptive stages on the serving path (risp_serve_scene.hip): gray-world, white-world and Reinhard need one
 * whole-image quantity in front of them - three sums, three maxima, one sum of logarithms.  The mosaic is read twice
 * instead of fp32 planes being written: a statistics launch, a finish launch, the serving launch (2 S + 1 launches for S
 * scene stages; the second statistics launch of a two-scene pipeline runs its prefix through the first scene stage).
 *
 * risp_serve_scene_stats: risp_serve_classical_u8's pixel pipeline (same arguments, rules, loads, reflection, phase and
 * black level) with the n_ops PREFIX stages; no image is stored.  The values behind the prefix are reduced per workgroup
 * (a 64 x 32 pixel tile) according to stat:
 *   RISP_SCENE_MEAN3   the sums of B, G, R of the [0,1] values                                          (gray-world)
 *   RISP_SCENE_MAX3    the maxima of B, G, R                                                            (white-world)
 *   RISP_SCENE_LOGLUM  the sum of log((0.114 b' + 0.587 g' + 0.299 r') / 255 + 1e-4), c' = max(c * 255, 0)  (Reinhard)
 * in a fixed order (the thread's eight pixels, wavefront shuffles, one LDS step; no atomics), and workgroup `tile` of image
 * n writes the row partials[(n * G + tile) * 4 .. + 3] = (B, G, R, 0) or (sum, 0, 0, 0), G = risp_serve_scene_groups(H, W),
 * tile = row-major index of the tiles of the mirrored image (the RGGB image of RISP_CFA_*: with cfa & 1 tile 0 holds the
 * sensor's right-most columns, with cfa & 2 its bottom rows; the remap of workgroups to XCDs does not enter).  Every row is written in full: partials (N,G,4) needs no initialisation.
 * Rules beyond risp_serve_classical_u8's: stat one of the three; partials not NULL and 16-byte aligned; ops[k] may also be
 * RISP_OP_GAIN3_Q8 / RISP_OP_TONE_REINHARD, whose params[k] is the 16-byte aligned consts of an earlier finish.
 *
 * risp_serve_scene_finish: consts from partials, one workgroup per image; the G rows are added (or maximised) in index
 * order in double precision and rounded to float once.  a, b: (N) per-image plugin parameters as risp_origin_tonemap takes
 * them.  A mean is the total times the reciprocal 1.0f / HW taken in fp32, as risp_grayworld_gains_fwd and risp_origin_tonemap
 * form it (not a division by HW).  consts holds 4 N floats, 16-byte aligned, every one written:
 *   MEAN3   gain_c = gray / max(mean_c, 1e-6), gray = the mean of the three means (risp_grayworld_gains_fwd's expression);
 *           stored as the (N,3) block RISP_OP_GAIN3 takes, packed in the first 3 N floats (the last N are 0).  a, b unused.
 *   MAX3    (N,4) rows (g_b, g_g, g_r, 0), g_c = 1 + a[n] (big / mx_c - 1), mx_c = max(max_c * 255, 1e-3), big = max mx_c;
 *           a = ratio (risp_origin_tonemap mode 3).  For RISP_OP_GAIN3_Q8.
 *   LOGLUM  (N,4) rows (p0, p1, 0, 0), p0 = max(b[n], 0.01) / exp(sum / HW), p1 = 1 / lw^2, lw = max(a[n], 0.01) * 10;
 *           a = white_point, b = middle_grey (risp_origin_tonemap mode 0).  For RISP_OP_TONE_REINHARD.
 * Rules: stat one of the three; partials, consts not NULL and 16-byte aligned; a not NULL but for MEAN3, b not NULL for
 * LOGLUM; 1 <= N <= 65535, G >= 1 (the statistics launch's), HW >= 1 (H * W).
 *
 * risp_serve_scene_u8: risp_serve_classical_u8 - signature, rules, bytes for the stages both accept - with two more
 * stages, which belong to this entry point (and to the prefix of risp_serve_scene_stats) alone:
 *   RISP_OP_GAIN3_Q8       white-world apply: risp_origin_tonemap mode 3's pixel expression with both scales 255 - the
 *                          value times its channel's gain, rounded to its 8-bit code / 255; params[k] = MAX3 consts
 *   RISP_OP_TONE_REINHARD  risp_origin_tonemap mode 0's pixel expression with both scales 255; params[k] = LOGLUM consts
 * Gray-world applies as RISP_OP_GAIN3 with the MEAN3 consts.  A pipeline whose only scene stages are white-world has the
 * composed route's bytes (a maximum has no order); sums taken in this order give constants that differ from the composed
 * route's in their last bits, so gray-world and Reinhard agree with it up to rounding ties only.
 * Anything outside the rules is refused before a launch and the message names the value. */
#define RISP_OP_GAIN3_Q8 9
#define RISP_OP_TONE_REINHARD 10
#define RISP_SCENE_MEAN3 0
#define RISP_SCENE_MAX3 1
#define RISP_SCENE_LOGLUM 2
int risp_serve_scene_groups(int H, int W); /* workgroups (partial rows) per image; 0 when H, W break the rules */
int risp_serve_scene_stats(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                           const float *const *params, int stat, float *partials, int N, int H, int W, int black_level,
                           int cfa, void *stream);
int risp_serve_scene_finish(int stat, const float *partials, const float *a, const float *b, float *consts, int N, int G,
                            int HW, void *stream);
int risp_serve_scene_u8(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                        const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W,
                        int black_level, int cfa, void *stream);

/* Conditional heads on the serving path (risp_serve_cond.hip): ConditionalGamma / ConditionalWbManual / ConditionalWbQuadratic
 * predict their parameters per image with an MLP on the per-channel histogram of their input.  The mosaic is read once more
 * per head instead of fp32 planes being written: a histogram launch, a finish launch, and risp_serve_classical_u8 serves with
 * the head as RISP_OP_GAMMA / WB_MANUAL / WB_QUADRATIC and the finished block (2 S + 1 launches for S heads; the histogram
 * launch of a later head runs its prefix through the earlier ones).
 *
 * risp_serve_cond_hist: risp_serve_classical_u8's pixel pipeline (same arguments, rules, loads, reflection, phase and black
 * level) with the n_ops PREFIX stages; no image is stored.  Every value v behind the prefix - B, G, R of every pixel - is
 * binned by risp_histc's rule: it counts only if v >= 0 && v <= 1 (NaN and values outside count nowhere), in bin
 * min((int)(v * (float)bins), bins - 1).  counts is (N, RISP_COND_SHARDS, 3 * bins) unsigned 32-bit integers, channel order
 * B, G, R: a workgroup (a 64 x 32 pixel tile) counts in private LDS histograms and adds its totals to shard
 * tile % RISP_COND_SHARDS of its image with integer atomics, so no result depends on an order; the histogram of image n is the
 * sum of its shards.  The entry point zeroes counts itself on the same stream (capturable): counts is fully defined after the
 * call whatever it held before.  Rules (anything else is refused before a launch and the message names the value): raw and
 * counts not NULL, raw 8-byte aligned, whole contiguous frames; divisor > 0; demosaic 0 .. 2; cfa 0 .. 3 and no mirrored axis
 * of odd length; 0 <= black_level <= 65535; bins >= 1 and 3 * bins <= 1024 (the widest layer of risp_cond_fc_fwd);
 * 1 <= N <= 65535, H even and >= 4, W % 4 == 0 and >= 4, H * W <= 2^24 (above it the float counts of risp_histc stop being
 * exact and "the composed route's bytes" cannot be promised); 0 <= n_ops <= RISP_MAX_CHAIN, ops[k] one of SKIP, WB_MANUAL ..
 * TONE_FILMIC as risp_serve_classical_u8 takes them, every stage but a SKIP needs params[k].
 *
 * risp_serve_cond_finish: one workgroup per image.  Word i of the image's `shards` rows of counts, added in integers and
 * converted to float once, is the histogram risp_histc gives; then risp_cond_fc_fwd's arithmetic on flat / widths / n_layers
 * (same expressions in the same order: z = sum_i a[i] W[i][j] in i order, + b[j], ReLU between layers, on the last layer
 * + the global scalar and 1 / (1 + exp(-z))), and block[n][j] = that value * scale in fp32 (scale 1: the value itself; 5 for
 * ConditionalWbManual).  block is (N, widths[n_layers]); no activation row is written.  Rules: counts, flat, block not NULL;
 * 1 <= shards <= 65535; 1 <= N <= 65535; scale > 0 and finite; 1 <= n_layers <= 8, every width in 1 .. 1024; counts rows are
 * widths[0] words long.  With both, the block - and every byte risp_serve_classical_u8 serves with it - is the composed
 * route's (risp_raw_crop_cfa -> ... -> risp_histc -> risp_cond_fc_fwd -> * scale). */
#define RISP_COND_SHARDS 32
int risp_serve_cond_hist(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                         const float *const *params, int bins, unsigned int *counts, int N, int H, int W, int black_level,
                         int cfa, void *stream);
int risp_serve_cond_finish(const unsigned int *counts, int shards, const float *flat, const int *widths, int n_layers,
                           float scale, float *block, int N, void *stream);

/* A classical pipeline with ONE classical denoiser as an ISP, one launch (risp_serve_denoise.hip): raw (N,H,W) uint16 mosaic
 * of the sensor -> out (N,H,W,3) bytes.  Per pixel: risp_serve_classical_u8's input expression and demosaic, the n_pre stages
 * pre_ops, the denoiser, the n_post stages post_ops, the conversion of risp_quantise_u8.  Only the result is stored; its bytes
 * are those of risp_raw_crop_cfa -> demosaic -> stages -> risp_origin_bilateral | risp_origin_median | risp_origin_fastnlm
 * (in_scale 255, out_div 255) -> stages -> risp_quantise_u8_flip, every stage as risp_serve_classical_u8 states it.
 * pre_ops[k], post_ops[k]: the stages risp_serve_classical_u8 accepts (SKIP, WB_MANUAL, GAMMA, GTM_MANUAL, WB_QUADRATIC, GAIN3,
 * TONE_CRYSIS, TONE_FILMIC), n_pre + n_post <= RISP_MAX_CHAIN, every stage but a SKIP needs its parameter block.
 * denoise: RISP_DENOISE_BILATERAL  window = 3, den_a = sigma_color (N), den_b = sigma_space (N); search ignored
 *          RISP_DENOISE_MEDIAN     window = 3 (the size); search, den_a, den_b ignored
 *          RISP_DENOISE_FASTNLM    window = 3 (the block), search = 3, den_a = decay (N); den_b ignored
 * with the per-image arrays as the risp_origin_* entry points take them.  Any other window, size, block or search is refused:
 * those pipelines compose.  The image border is reflect-101 in the image the denoiser sees (the pipeline evaluated at the
 * reflected coordinate), as in risp_origin_*.
 * A workgroup owns a 64 x 32 pixel tile: it evaluates demosaic and pre-stages for the tile and a ring into LDS (three fp32
 * planes of 36 x 72, 31104 bytes), one barrier (two on the image border), then the denoiser and post-stages per thread.
 * black_level and cfa as in risp_serve_u8_cfa.  Rules (anything else is refused before a launch and the message names it): raw
 * and out not NULL, raw 8-byte and out 4-byte aligned, whole contiguous frames; divisor > 0; demosaic 0 .. 2; denoise 0 .. 2;
 * 1 <= N <= 65535, H even and >= 4, W % 4 == 0 and >= 4; cfa 0 .. 3; 0 <= black_level <= 65535. */
#define RISP_DENOISE_BILATERAL 0
#define RISP_DENOISE_MEDIAN 1
#define RISP_DENOISE_FASTNLM 2
int risp_serve_denoise_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                          const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                          const float *den_b, int n_post, const int *post_ops, const float *const *post_params, uint8_t *out,
                          int reverse_channels, int N, int H, int W, int black_level, int cfa, void *stream);

/* risp_serve_denoise_u8's median at the other sizes OriginNoiseMedian's rule gives below a saturated parameter, one launch
 * (risp_serve_median.hip): raw (N,H,W) uint16 mosaic of the sensor -> out (N,H,W,3) bytes.  Per pixel: risp_serve_classical_u8's
 * input expression and demosaic, the n_pre stages pre_ops, the size x size median of the 8-bit codes, the n_post stages post_ops,
 * the conversion of risp_quantise_u8.  Only the result is stored; its bytes are those of risp_raw_crop_cfa -> demosaic -> stages ->
 * risp_origin_median (that size, in_scale 255, out_div 255) -> stages -> risp_quantise_u8_flip, every stage as
 * risp_serve_classical_u8 states it: the median is the smallest code whose rank among the size * size codes of the window reaches
 * size * size / 2 + 1, and the image border is reflect-101 in the image the median sees (the pipeline evaluated at the reflected
 * coordinate).  pre_ops[k], post_ops[k]: the stages risp_serve_classical_u8 accepts, n_pre + n_post <= RISP_MAX_CHAIN, every stage
 * but a SKIP needs its parameter block.
 * A workgroup owns a 64 x 32 pixel tile: it evaluates demosaic and pre-stages for the tile and a ring (size / 2 rounded up to even
 * rows, 4 columns up to size 9 and 8 above) into LDS as codes packed four to a dword (7776 .. 11520 bytes), one barrier (two on
 * the image border), then the median - byte windows in registers, rank counts by sums of absolute differences, a bisection on the
 * code - and the post-stages per thread.  black_level and cfa as in risp_serve_u8_cfa.
 * Rules (anything else is refused before a launch and the message names it): size 5, 7, 9, 11, 13 or 15 (3 is
 * risp_serve_denoise_u8's, 17 is not served); H even, >= 4 and > size / 2; W % 4 == 0 and > size / 2; and everything
 * risp_serve_denoise_u8 asks: raw and out not NULL, raw 8-byte and out 4-byte aligned, whole contiguous frames; divisor > 0;
 * demosaic 0 .. 2; 1 <= N <= 65535; cfa 0 .. 3; 0 <= black_level <= 65535. */
int risp_serve_median_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                         const float *const *pre_params, int size, int n_post, const int *post_ops,
                         const float *const *post_params, uint8_t *out, int reverse_channels, int N, int H, int W,
                         int black_level, int cfa, void *stream);

/* A classical denoiser beside gray-world / white-world on the serving path (risp_serve_denoise_scene.hip): the statistic of an
 * image that lies BEHIND a denoiser, and a serving launch that takes a denoiser and the scene constants together.  With
 * risp_serve_scene_stats (a scene stage whose prefix holds no denoiser) and risp_serve_scene_finish a pipeline with S scene stages
 * and one denoiser runs in 2 S + 1 launches and writes no fp32 plane.
 *
 * risp_serve_denoise_stats: risp_serve_denoise_u8's tile pipeline (same arguments, rules, loads, mosaic reflection, image-border
 * reflection, phase, black level, two-phase LDS tile of 31104 bytes) with the n_post stages behind the denoiser evaluated in
 * registers; no image is stored.  The values behind the last post stage are reduced per workgroup (a 64 x 32 pixel tile)
 * according to stat:
 *   RISP_SCENE_MEAN3   the sums of B, G, R of the [0,1] values        (gray-world)
 *   RISP_SCENE_MAX3    the maxima of B, G, R                          (white-world)
 * in risp_serve_scene_stats' order (the thread's eight pixels in row order, wavefront shuffles, one LDS step in wave order; no
 * atomics; a thread of a ragged tile that owns no pixel holds 0 for a sum and -inf for a maximum), and workgroup `tile` of image n
 * writes the row partials[(n * G + tile) * 4 .. + 3] = (B, G, R, 0), G = risp_serve_scene_groups(H, W), tile = row-major index of
 * the tiles of the mirrored (RGGB) image: exactly the layout of risp_serve_scene_stats, every row written in full, and
 * risp_serve_scene_finish turns the rows into constants unchanged.  RISP_SCENE_LOGLUM is refused.
 *
 * risp_serve_denoise_scene_u8: risp_serve_denoise_u8 - signature, rules, bytes for every stage both accept - with one more stage
 * accepted in front of and behind the denoiser:
 *   RISP_OP_GAIN3_Q8   white-world apply, the expression risp_serve_scene_u8 has: the value times its channel's gain, rounded to
 *                      its 8-bit code / 255; its parameter block is the 16-byte aligned MAX3 consts of risp_serve_scene_finish
 * Gray-world applies as the existing RISP_OP_GAIN3 with the MEAN3 consts.  RISP_OP_TONE_REINHARD is refused by both entry points
 * (its log-average has no order-free form and its apply step no stand-alone entry point to be held to).  The prefix of
 * risp_serve_denoise_stats accepts RISP_OP_GAIN3_Q8 too: an earlier scene stage enters it with its constants.
 *
 * Contract.  Given the constants, the bytes are those of the composed route evaluated with the same constants
 * (risp_raw_crop_cfa -> demosaic -> stages -> risp_origin_* -> stages -> risp_quantise_u8_flip, gray-world as risp_gain3_fwd and
 * white-world as risp_origin_tonemap mode 3 at their places).  A maximum has no order: MAX3 rows, white-world's constants and the
 * bytes of a pipeline whose only scene stages are white-world are the composed route's.  A sum taken in this order differs from
 * risp_channel_stats' in its last bits: a MEAN3 row lies within (64 * 32 - 1) * 2^-24 * sum|x| of the exact sum of its tile.
 *
 * Rules for both (anything else is refused before a launch and the message names the value): those of risp_serve_denoise_u8 -
 * bilateral window 3, median size 3, non-local means block 3 and search 3, the denoiser's parameter blocks; H even and >= 4,
 * W % 4 == 0 and >= 4, 1 <= N <= 65535; n_pre + n_post <= RISP_MAX_CHAIN; every stage but a SKIP needs its parameter block; raw
 * 8-byte aligned; divisor > 0; demosaic 0 .. 2; denoise 0 .. 2; cfa 0 .. 3; 0 <= black_level <= 65535 - plus stat MEAN3 or MAX3 and
 * partials not NULL and 16-byte aligned (the statistics), out not NULL and 4-byte aligned (the serving launch). */
int risp_serve_denoise_stats(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                             const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                             const float *den_b, int n_post, const int *post_ops, const float *const *post_params, int stat,
                             float *partials, int N, int H, int W, int black_level, int cfa, void *stream);
int risp_serve_denoise_scene_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                                const float *den_b, int n_post, const int *post_ops, const float *const *post_params, uint8_t *out,
                                int reverse_channels, int N, int H, int W, int black_level, int cfa, void *stream);

/* Diagnostics: the kernel instance risp_bilateral_chain_fwd launches for these arguments (16-byte aligned input), named as rocprofv3 prints it
 * (bench.py binds the committed counter readings of profiles/traffic.json to the kernel it actually launches). */
const char *risp_bilateral_chain_kernel(int from_bayer, int max_window, int with_wb_quadratic);

#ifdef __cplusplus
}
#endif
#endif /* RISP_H */
