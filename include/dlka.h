/*
 * dlka.h — C-ABI of libdlka_hip.so: the MI355X (gfx950) implementation of the Deformable
 * Large-Kernel-Attention hot path of xmindflow/deformableLKA.
 *
 * This is the drop-in boundary.  Every entry point takes plain device pointers, a geometry
 * struct of ints and an opaque hipStream_t; no torch / ATen type crosses it.  Each declaration
 * cites the reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers to dense, contiguous buffers in the layouts stated
 *     per function (the reference asserts contiguity: 3D/dcn/src/cuda/deform_conv_cuda.cu:41-42).
 *   - Inputs are borrowed and never written.  Outputs and workspaces are caller-allocated
 *     (the reference allocates outputs itself with at::empty/zeros_like, deform_conv_cuda.cu:82,
 *     202-205; here the host-language wrapper owns allocation so that the library stays ATen-free).
 *   - Every call is asynchronous on `stream` (the reference uses the current CUDA stream,
 *     deform_conv_cuda.cu:97) and is legal inside hipGraph capture: no allocation, no sync.
 *   - Return value: DLKA_OK (0) or a negative dlka_status.  Nothing throws across this boundary.
 *     dlka_status_string() gives the message the Python wrapper turns into RuntimeError, matching
 *     the reference's AT_ASSERTM -> c10::Error -> RuntimeError behaviour.
 *   - dtype: DLKA_F32 everywhere (the reference dispatches float/double only,
 *     deform_conv_cuda.cu:96,233).  DLKA_BF16 = bf16 storage with fp32 accumulation (new capability).
 */
#ifndef DLKA_H_
#define DLKA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLKA_ABI_VERSION 1

typedef enum dlka_status {
    DLKA_OK = 0,
    DLKA_ERR_NULL = -1,         /* a required pointer is NULL                                          */
    DLKA_ERR_GROUP = -2,        /* channels / out_channels not divisible by group (cu:65-66)           */
    DLKA_ERR_DEFORM_GROUP = -3, /* channels not divisible by deformable_group                          */
    DLKA_ERR_SHAPE = -4,        /* non-positive size or output size (cu:78-80)                         */
    DLKA_ERR_IM2COL_STEP = -5,  /* batch % min(batch, im2col_step) != 0 (cu:61-63)                      */
    DLKA_ERR_DTYPE = -6,        /* unsupported dtype                                                    */
    DLKA_ERR_WORKSPACE = -7,    /* workspace too small / NULL                                           */
    DLKA_ERR_UNSUPPORTED = -8,  /* parameter combination not implemented                                */
    DLKA_ERR_LAUNCH = -9        /* hipGetLastError() != hipSuccess after a launch (reference only printf's, cuh:425-429) */
} dlka_status;

/* DLKA_F64: the reference's op dispatches float AND double (AT_DISPATCH_FLOATING_TYPES, 3D/dcn/src/cuda/deform_conv_cuda.cu:96,233; its scripts import gradcheck,
 * 3D/dcn/test.py:9).  Accepted by the GENERAL NCDHW entry points — dlka_deform_conv3d_*, dlka_deform_conv2d_*, dlka_conv3d_* (forward, backward; every tensor double) —
 * and nowhere else: the fused blocks and the channels-last fast paths return DLKA_ERR_DTYPE / DLKA_ERR_UNSUPPORTED for it. */
typedef enum dlka_dtype { DLKA_F32 = 0, DLKA_BF16 = 1, DLKA_F64 = 2 } dlka_dtype;

/* Geometry of one (deformable or plain) N-d convolution.  2-D ops use D = kd = sd = dd = 1, pd = 0. */
typedef struct dlka_conv_geom {
    int32_t B, C, D, H, W;     /* input  [B][C][D][H][W]                                  */
    int32_t Cout;              /* weight [Cout][C/group][kd][kh][kw]                      */
    int32_t kd, kh, kw;
    int32_t sd, sh, sw;        /* stride                                                  */
    int32_t pd, ph, pw;        /* zero padding                                            */
    int32_t dd, dh, dw;        /* dilation                                                */
    int32_t group;             /* weight groups                                           */
    int32_t deformable_group;  /* offset groups (deformable ops only; else ignored)       */
    int32_t im2col_step;       /* accepted and validated for API parity only (cu:59-63);
                                  no column buffer exists here, so it does not change the result */
} dlka_conv_geom;

int         dlka_abi_version(void);
const char *dlka_status_string(int status);
/* Output spatial size  (in + 2p - (d(k-1)+1))/s + 1   (deform_conv_cuda.cu:78-80). */
int         dlka_conv_out_size(int in, int pad, int dil, int k, int stride);

/* =======================================================================================
 * 3-D deformable convolution — the D3D operator
 * ======================================================================================= */

/* Replaces  D3D.deform_conv_forward  (3D/dcn/src/vision.cpp:5, 3D/dcn/src/deform_conv.h:10-47)
 *           = deform_conv_cuda_forward (3D/dcn/src/cuda/deform_conv_cuda.cu:18-126)
 *           + deformable_im2col_gpu_kernel (3D/dcn/src/cuda/deform_im2col_cuda.cuh:192-265).
 *   x      [B][C][D][H][W]
 *   offset [B][dg*3*K][Do][Ho][Wo]   channel = dg_idx*3K + 3*tap + {0:d,1:h,2:w}, tap=(i*kh+j)*kw+k (cuh:237-239)
 *   weight [Cout][C/group][kd][kh][kw]
 *   bias   [Cout]                    always added, also when the module was built with bias=False
 *   out    [B][Cout][Do][Ho][Wo]
 *   workspace: dlka_deform_conv3d_forward_workspace(g, dtype) bytes (re-laid-out weights; no im2col columns). */
size_t dlka_deform_conv3d_forward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_deform_conv3d_forward(const void *x, const void *offset, const void *weight, const void *bias,
                               void *out, void *workspace, size_t workspace_bytes,
                               const dlka_conv_geom *g, int dtype, void *stream);

/* Replaces  D3D.deform_conv_backward (3D/dcn/src/vision.cpp:6, deform_conv.h:49-91)
 *           = deform_conv_cuda_backward (deform_conv_cuda.cu:128-285)
 *           + deformable_col2im_coord_gpu_kernel (cuh:336-405)  -> grad_offset
 *           + deformable_col2im_gpu_kernel       (cuh:267-334)  -> grad_x   (fp32 atomics, order non-deterministic as in the reference)
 *           + deformable_im2col_gpu_kernel again + addmm/addmv (cu:254-278) -> grad_weight, grad_bias.
 *   All four gradients are fully overwritten (the reference returns fresh zeros_like tensors, cu:202-205).
 *   Any of the grad_* pointers may be NULL to skip that gradient. */
size_t dlka_deform_conv3d_backward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_deform_conv3d_backward(const void *x, const void *offset, const void *weight, const void *grad_out,
                                void *grad_x, void *grad_offset, void *grad_weight, void *grad_bias,
                                void *workspace, size_t workspace_bytes,
                                const dlka_conv_geom *g, int dtype, void *stream);

/* Debug/parity entry point: floor() sampling indices and the in-range guard of cuh:247 for every
 * (b, dg, tap, out voxel).  idx int32 [B][dg][K][No][3], mask uint8 [B][dg][K][No].
 * Backs the "integer sampling indices bit-exact" requirement of BASELINE.json. */
int dlka_deform_conv3d_sample_index(const void *offset, int32_t *idx, uint8_t *mask,
                                    const dlka_conv_geom *g, int dtype, void *stream);
/* Same outputs, computed by the very device functions the hot kernels call, so that the bit-exact index claim covers
 * the code that runs.  ONE device function forms q, tests the guard and takes the floor (sample_cell3, deform_sample.h);
 * path 0 = that function on its own (cl_deform_gx_fx2_kernel calls it directly); path 1 = setup_tap<3> (every general NCDHW
 * kernel); path 2 = gather_describe3 (cl_gather.h — the channels-last forward / grad_offset / weight-gradient kernels);
 * path 3 = lane_tap (the grad_input window kernels).  idx = 0 where mask == 0 (outside the guard of cuh:247 no cell is formed). */
int dlka_deform_conv3d_sample_index_path(const void *offset, int32_t *idx, uint8_t *mask,
                                         const dlka_conv_geom *g, int dtype, int path, void *stream);

/* =======================================================================================
 * 2-D deformable convolution — torchvision.ops.deform_conv2d(mask=None) semantics
 * ======================================================================================= */

/* Replaces  torchvision.ops.DeformConv2d.forward / deform_conv2d as called at
 *           2D/deformable_LKA/deformable_LKA.py:18-30 (torchvision==0.12.0, 2D/requirements.txt:69).
 *   x [B][C][H][W]; offset [B][og*2*K][Ho][Wo] with (dy,dx) per tap; weight [Cout][C/group][kh][kw];
 *   bias [Cout] or NULL (the reference passes bias=False, deformable_LKA.py:25); out [B][Cout][Ho][Wo].
 *   Geometry: D=kd=sd=dd=1, pd=0; deformable_group = offset groups. */
size_t dlka_deform_conv2d_forward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_deform_conv2d_forward(const void *x, const void *offset, const void *weight, const void *bias,
                               void *out, void *workspace, size_t workspace_bytes,
                               const dlka_conv_geom *g, int dtype, void *stream);
size_t dlka_deform_conv2d_backward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_deform_conv2d_backward(const void *x, const void *offset, const void *weight, const void *grad_out,
                                void *grad_x, void *grad_offset, void *grad_weight, void *grad_bias,
                                void *workspace, size_t workspace_bytes,
                                const dlka_conv_geom *g, int dtype, void *stream);

/* =======================================================================================
 * Plain grouped N-d convolution — the nn.Conv3d / nn.Conv2d calls that sit on the path
 * ======================================================================================= */

/* Replaces the cuDNN-backed nn.Conv3d / nn.Conv2d modules inside the D-LKA block:
 *   depthwise 5^3 pad 2 and 7^3 dil 3 pad 9   (3D/d_lka_former/network_architecture/synapse/transformerblock.py:637-638)
 *   offset-predict conv C->81, 3^3 pad 1      (3D/d_lka_former/network_architecture/synapse/deform_conv.py:80-85)
 *   1x1x1 convs proj_1 / conv1 / proj_2       (transformerblock.py:641,659,662)
 *   2-D offset nets C->50 (5x5) / C->98 (7x7 dil 3) (2D/deformable_LKA/deformable_LKA.py:10-16)
 *   x [B][C][D][H][W]; weight [Cout][C/group][kd][kh][kw]; bias [Cout] or NULL; out [B][Cout][Do][Ho][Wo]. */
size_t dlka_conv3d_forward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_conv3d_forward(const void *x, const void *weight, const void *bias, void *out,
                        void *workspace, size_t workspace_bytes,
                        const dlka_conv_geom *g, int dtype, void *stream);
/* grad_x / grad_weight / grad_bias may each be NULL to skip. All are fully overwritten.
 * Arithmetic (DLKA_F32): fp32 products and sums — except the shape the assembled net's full-resolution plumbing uses (3^3, stride 1, padding 1, group 1, <= 16 -> <= 16
 * channels, W % 8 == 0): its grad_x (W <= 128, >= 8 output channels) and grad_weight contract on the bf16 matrix cores with BOTH operands as two bf16 terms and fp32
 * accumulation (~1e-5 of max|gradient|, inside the 1e-3 gradient contract; the rule of the token-layout block's gradients, see dlka_lka3d_attention_tokens_backward).
 * DLKA_EXACT_FP32=1 keeps fp32-input MFMAs there too. */
size_t dlka_conv3d_backward_workspace(const dlka_conv_geom *g, int dtype);
int dlka_conv3d_backward(const void *x, const void *weight, const void *grad_out,
                         void *grad_x, void *grad_weight, void *grad_bias,
                         void *workspace, size_t workspace_bytes,
                         const dlka_conv_geom *g, int dtype, void *stream);

/* =======================================================================================
 * Elementwise pieces of the block (GELU, gate)
 * ======================================================================================= */

/* y = GELU_erf(x)  (nn.GELU() default, transformerblock.py:660);  n elements. */
int dlka_gelu_forward(const void *x, void *y, int64_t n, int dtype, void *stream);
/* gx = gy * dGELU(x) */
int dlka_gelu_backward(const void *x, const void *gy, void *gx, int64_t n, int dtype, void *stream);
/* y = a * b   (the "u * attn" gate, transformerblock.py:652; deformable_LKA.py:104) */
int dlka_mul_forward(const void *a, const void *b, void *y, int64_t n, int dtype, void *stream);
/* ga = gy * b ; gb = gy * a */
int dlka_mul_backward(const void *a, const void *b, const void *gy, void *ga, void *gb, int64_t n, int dtype, void *stream);
/* y = a + b */
int dlka_add_forward(const void *a, const void *b, void *y, int64_t n, int dtype, void *stream);

/* =======================================================================================
 * Whole D-LKA attention blocks (fused launch sequences; one C call per block)
 * ======================================================================================= */

/* Parameters of LKA_Attention3d_deform (transformerblock.py:655-673) in state_dict order. All [..] dense. */
typedef struct dlka_lka3d_params {
    const void *proj_1_w, *proj_1_b;             /* [C][C][1][1][1], [C]              proj_1                         */
    const void *conv0_w, *conv0_b;               /* [C][1][5][5][5], [C]              spatial_gating_unit.conv0       */
    const void *conv_spatial_w, *conv_spatial_b; /* [C][1][7][7][7], [C]              spatial_gating_unit.conv_spatial */
    const void *offset_w, *offset_b;             /* [81][C][3][3][3], [81]            ...deform_conv.conv_offset      */
    const void *deform_w, *deform_b;             /* [C][C][3][3][3], [C]              ...deform_conv.{weight,bias}    */
    const void *conv1_w, *conv1_b;               /* [C][C][1][1][1], [C]              spatial_gating_unit.conv1       */
    const void *proj_2_w, *proj_2_b;             /* [C][C][1][1][1], [C]              proj_2                         */
} dlka_lka3d_params;

typedef struct dlka_lka3d_grads { /* same shapes as dlka_lka3d_params; all fully overwritten */
    void *proj_1_w, *proj_1_b, *conv0_w, *conv0_b, *conv_spatial_w, *conv_spatial_b, *offset_w, *offset_b,
         *deform_w, *deform_b, *conv1_w, *conv1_b, *proj_2_w, *proj_2_b;
} dlka_lka3d_grads;

/* Replaces  LKA_Attention3d_deform.forward(x, B, C, H, W, D)  (transformerblock.py:664-673) including
 *           LKA3d_deform.forward (:644-652) and DeformConvPack.forward (synapse/deform_conv.py:93-105).
 *   x, y: NCDHW volumes [B][C][D][H][W] (the (B,N,C)<->NCDHW permutes of :665,672 stay in the caller:
 *   they are views/copies on the Python side exactly as in the reference).
 *   saved: activations the backward needs; dlka_lka3d_saved_bytes(B,C,D,H,W,dtype) bytes, caller-owned,
 *          must stay untouched until the matching backward call.
 *   workspace: scratch, dlka_lka3d_workspace_bytes(...) bytes, may be reused right after the call. */
size_t dlka_lka3d_saved_bytes(int B, int C, int D, int H, int W, int dtype);
size_t dlka_lka3d_workspace_bytes(int B, int C, int D, int H, int W, int dtype);
int dlka_lka3d_attention_forward(const void *x, const dlka_lka3d_params *p, void *y,
                                 void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                                 int B, int C, int D, int H, int W, int dtype, void *stream);
/* Backward of the above: grad_y -> grad_x and all 14 parameter gradients. */
int dlka_lka3d_attention_backward(const void *x, const dlka_lka3d_params *p, const void *grad_y,
                                  const void *saved, size_t saved_bytes,
                                  void *grad_x, const dlka_lka3d_grads *grads,
                                  void *workspace, size_t workspace_bytes,
                                  int B, int C, int D, int H, int W, int dtype, void *stream);

/* Parameters of the 2-D deformable_LKA_Attention (2D/deformable_LKA/deformable_LKA.py:124-140). */
typedef struct dlka_lka2d_params {
    const void *proj_1_w, *proj_1_b;             /* [C][C][1][1], [C]                                             */
    const void *conv0_offset_w, *conv0_offset_b; /* [50][C][5][5], [50]   conv0.offset_net                         */
    const void *conv0_w;                         /* [C][1][5][5]          conv0.deform_conv.weight (bias=False)    */
    const void *conv_spatial_offset_w, *conv_spatial_offset_b; /* [98][C][7][7], [98]  conv_spatial.offset_net      */
    const void *conv_spatial_w;                  /* [C][1][7][7]          conv_spatial.deform_conv.weight          */
    const void *conv1_w, *conv1_b;               /* [C][C][1][1], [C]                                             */
    const void *proj_2_w, *proj_2_b;             /* [C][C][1][1], [C]                                             */
} dlka_lka2d_params;

typedef struct dlka_lka2d_grads {
    void *proj_1_w, *proj_1_b, *conv0_offset_w, *conv0_offset_b, *conv0_w,
         *conv_spatial_offset_w, *conv_spatial_offset_b, *conv_spatial_w, *conv1_w, *conv1_b, *proj_2_w, *proj_2_b;
} dlka_lka2d_grads;

/* Replaces  deformable_LKA_Attention.forward (deformable_LKA.py:133-140) incl. deformable_LKA.forward (:98-104)
 *           and DeformConv.forward (:27-30).  x, y: [B][C][H][W]. */
/* dtype DLKA_BF16 (BASELINE.json config 2, "bf16 training"): x / y / grad_y / grad_x and the saved activations are bf16 storage, the
 * PARAMETERS and their gradients stay fp32 masters, offsets and accumulation are fp32, and the chain that decides the sampling cells
 * (a -> offset net 5 -> DDW5 -> offset net 7) is kept in fp32.  Channels-last fast path only: C / 32 in {1, 2, 3, 4, 6, 8, 12};
 * other widths return DLKA_ERR_UNSUPPORTED for DLKA_BF16. */
size_t dlka_lka2d_saved_bytes(int B, int C, int H, int W, int dtype);
size_t dlka_lka2d_workspace_bytes(int B, int C, int H, int W, int dtype);
int dlka_lka2d_attention_forward(const void *x, const dlka_lka2d_params *p, void *y,
                                 void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                                 int B, int C, int H, int W, int dtype, void *stream);
/* Forces (1) / releases (0) the general NCHW kernels for blocks the channels-last fast path would take; returns the previous setting.  Initial
 * value: 1 iff the environment variable DLKA_LKA2D_GENERAL is set when the first 2-D block call is made.  For A/B runs and the parity test of
 * one path against the other; the size queries return the maximum over both paths, so a switch never under-sizes a buffer. */
int dlka_lka2d_force_general(int on);
/* Diagnostics (bench health check, the parity tests' cell-flip analysis): where inside the opaque `saved` buffer of a forward call the two
 * predicted offset tensors live — conv0's [B][50][H][W] and conv_spatial's [B][98][H][W], planar as torchvision lays them out — for the path a
 * call with these arguments takes NOW (fast / general, see dlka_lka2d_force_general).  byte_offsets[0..1]: byte offsets from `saved`;
 * *elem_bytes: 4 (fp32; always on the channels-last path) or 2 (general path with bf16 tensors). */
int dlka_lka2d_saved_offsets(int B, int C, int H, int W, int dtype, size_t byte_offsets[2], int *elem_bytes);
int dlka_lka2d_attention_backward(const void *x, const dlka_lka2d_params *p, const void *grad_y,
                                  const void *saved, size_t saved_bytes,
                                  void *grad_x, const dlka_lka2d_grads *grads,
                                  void *workspace, size_t workspace_bytes,
                                  int B, int C, int H, int W, int dtype, void *stream);

/* Parameters of the plain (non-deformable) 2-D LKA_Attention (2D/deformable_LKA/LKA.py:4-37; the same block as SpatialAttention /
 * AttentionModule of 2D/networks/MaxViT_LKA_Decoder.py:53-85).  Unlike the deformable block, both depthwise convs carry a bias. */
typedef struct dlka_lka2d_plain_params {
    const void *proj_1_w, *proj_1_b;             /* [C][C][1][1], [C]                                             */
    const void *conv0_w, *conv0_b;               /* [C][1][5][5], [C]     spatial_gating_unit.conv0                */
    const void *conv_spatial_w, *conv_spatial_b; /* [C][1][7][7], [C]     spatial_gating_unit.conv_spatial (dil 3) */
    const void *conv1_w, *conv1_b;               /* [C][C][1][1], [C]                                             */
    const void *proj_2_w, *proj_2_b;             /* [C][C][1][1], [C]                                             */
} dlka_lka2d_plain_params;

typedef struct dlka_lka2d_plain_grads {
    void *proj_1_w, *proj_1_b, *conv0_w, *conv0_b, *conv_spatial_w, *conv_spatial_b, *conv1_w, *conv1_b, *proj_2_w, *proj_2_b;
} dlka_lka2d_plain_grads;

/* Replaces  LKA_Attention.forward (LKA.py:30-37) incl. LKA.forward (:12-18):  y = proj_2(u * conv1(conv_spatial(conv0(u)))) + x,  u = GELU(proj_1 x).
 * x, y: [B][C][H][W]; the block runs channels-last inside.  dtype DLKA_F32, or DLKA_BF16: x / y / grad_y / grad_x and the saved activations are bf16
 * storage, the PARAMETERS and their gradients stay fp32 masters, accumulation is fp32.  Covered: C / 32 in {1, 2, 3, 4, 6, 8, 12}; for anything else the
 * size queries return 0 and the calls DLKA_ERR_UNSUPPORTED (the modules then run operator by operator).  No float atomics: two identical calls give the
 * same bits.  saved / workspace: as for dlka_lka2d_attention_*. */
size_t dlka_lka2d_plain_saved_bytes(int B, int C, int H, int W, int dtype);
size_t dlka_lka2d_plain_workspace_bytes(int B, int C, int H, int W, int dtype);
int dlka_lka2d_plain_attention_forward(const void *x, const dlka_lka2d_plain_params *p, void *y,
                                       void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                                       int B, int C, int H, int W, int dtype, void *stream);
int dlka_lka2d_plain_attention_backward(const void *x, const dlka_lka2d_plain_params *p, const void *grad_y,
                                        const void *saved, size_t saved_bytes,
                                        void *grad_x, const dlka_lka2d_plain_grads *grads,
                                        void *workspace, size_t workspace_bytes,
                                        int B, int C, int H, int W, int dtype, void *stream);
/* The block's two depthwise convs as single operators, channels-last (cl_dw2d.hip): x / out / grad_out / grad_x [B][H][W][C] (float, or bf16 storage
 * with DLKA_BF16), weight / grad_weight [C][1][k][k] and bias / grad_bias [C] always fp32.  geom: D = kd = 1, stride 1, group = Cout = C, C % 32 == 0,
 * (k, dilation, padding) = (5, 1, 2) or (7, 3, 9); anything else DLKA_ERR_UNSUPPORTED.  bias may be null.  backward: grad_x / grad_weight optional
 * (null = not wanted), grad_bias needs grad_weight.  The weight and bias gradients are summed in a fixed order (no atomics). */
size_t dlka_dwconv2d_cl_workspace(const dlka_conv_geom *geom, int dtype, int backward);
int dlka_dwconv2d_forward_cl(const void *x, const void *weight, const void *bias, void *out, void *workspace, size_t workspace_bytes,
                             const dlka_conv_geom *geom, int dtype, void *stream);
int dlka_dwconv2d_backward_cl(const void *x, const void *weight, const void *grad_out, void *grad_x, void *grad_weight, void *grad_bias,
                              void *workspace, size_t workspace_bytes, const dlka_conv_geom *geom, int dtype, void *stream);


/* =======================================================================================
 * Channels-last (NDHWC / token layout) fast path — fp32, stride 1, same-size output
 * ======================================================================================= *
 * The D-LKA block's real interface is the token tensor (B, N, C) (transformerblock.py:664-673): the reference permutes
 * it to NCDHW (a copy), runs the block, and permutes back (another copy).  On MI355X the whole block runs directly in
 * token = channels-last layout: dense contractions (1x1x1 projections, offset-predict conv, deformable conv and their
 * gradients) are implicit GEMMs on the fp32-input matrix cores, depthwise convs are register-tiled vector kernels.
 * Offsets keep the reference's planar layout [B][3K][N].  Functions return DLKA_ERR_UNSUPPORTED for shapes outside
 * the fast path (caller then uses the general NCDHW entry points above).                                              */

/* x [B][D][H][W][C]; weight/bias in the reference layout; out [B][D][H][W][Cout], or planar [B][Cout][N] if out_planar.
 * Depthwise (group == C == Cout, kw/dilation in {5/1, 7/3, 3/1, 5/3, 7/1}) or dense (group == 1, C % 32 == 0). */
size_t dlka_conv3d_cl_workspace(const dlka_conv_geom *g, int dtype, int backward);
int dlka_conv3d_forward_cl(const void *x, const void *weight, const void *bias, void *out, int out_planar,
                           void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);
int dlka_conv3d_backward_cl(const void *x, const void *weight, const void *grad_out, int grad_out_planar,
                            void *grad_x, void *grad_weight, void *grad_bias,
                            void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);

/* Deformable conv with x / out / grad_x channels-last and offset / grad_offset planar (reference layout).
 * group == deformable_group == 1, C and Cout in {32, 64, 96, 128, 256}.  Same semantics as dlka_deform_conv3d_*.
 * dtype DLKA_F32, or DLKA_BF16 = MIXED storage: x / out / grad_out bf16; offset, weight, bias and ALL FOUR gradients fp32.  The arithmetic is fp32 (exact
 * products of the fp32 samples, fp32 accumulation, `out` rounded once at the store); backward refuses grad_bias without grad_weight for DLKA_BF16. */
size_t dlka_deform_conv3d_cl_workspace(const dlka_conv_geom *g, int dtype, int backward);
int dlka_deform_conv3d_forward_cl(const void *x, const void *offset, const void *weight, const void *bias, void *out,
                                  void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);
int dlka_deform_conv3d_backward_cl(const void *x, const void *offset, const void *weight, const void *grad_out,
                                   void *grad_x, void *grad_offset, void *grad_weight, void *grad_bias,
                                   void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);

/* [B][C][N] <-> [B][N][C] */
int dlka_ncdhw_to_ndhwc(const void *src, void *dst, int B, int C, int N, int dtype, void *stream);
int dlka_ndhwc_to_ncdhw(const void *src, void *dst, int B, int C, int N, int dtype, void *stream);

/* Replaces  LKA_Attention3d_deform.forward(x, B, C, H, W, D)  (transformerblock.py:664-673) on the TOKEN tensor itself:
 *   x, y, grad_x, grad_y: [B][N][C] with N = D*H*W voxels in (d,h,w) order of the reference's reshape(B,C,H,W,D)
 *   (its "H,W,D" are just the three spatial extents).  No permute/copy on either side.
 *   Supported: C in {32, 64, 128, 256} (the four D_LKA_Former stage widths); dtype
 *     DLKA_F32   everything fp32 storage and fp32 accumulation (the parity path: 1e-4 forward, 1e-3 gradients against the reference).  ARITHMETIC of the contractions:
 *                the FORWARD deformable conv and the pointwise convs run on the fp32-input MFMA (exact fp32 products); the forward offset-predict conv as a THREE-term
 *                bf16 split (six products per fp32 product: fp32-equivalent — its output decides floor()); the BACKWARD contractions of the deformable conv (Col of
 *                grad_offset / grad_input), its WEIGHT gradient (fp32 grad_out x the samples grad_offset handed over as IEEE halves — a half is exactly two bf16 terms; the halves are
 *                sample * 2^e with one e per call taken from max |t|, so the hand-over does not depend on the activations' scale, and Inf / NaN samples propagate)
 *                and the offset conv's data / weight gradients as TWO-term bf16 splits (three products, fp32 accumulation, ~1e-5 relative: inside the 1e-3 gradient
 *                contract).  DLKA_EXACT_FP32=1 (environment, read once) puts every contraction on the fp32-input MFMA (and keeps the samples fp32);
 *     DLKA_BF16  x, y, grad_y, grad_x and every saved / intermediate activation are bf16 STORAGE; parameters (dlka_lka3d_params), their
 *                gradients, the predicted offsets, grad_offset and all accumulation are fp32.  The offset-predict conv runs single bf16
 *                MFMA products against two-term (fp32-exact) weights.  The reference registers no autocast policy and would raise on half
 *                inputs (deform_conv_cuda.cu:96); this is the policy the Python modules apply inside torch.autocast(dtype=bfloat16). */
int    dlka_lka3d_tokens_supported(int B, int C, int D, int H, int W, int dtype);
size_t dlka_lka3d_tokens_saved_bytes(int B, int C, int D, int H, int W, int dtype);
size_t dlka_lka3d_tokens_workspace_bytes(int B, int C, int D, int H, int W, int dtype);
int dlka_lka3d_attention_tokens_forward(const void *x, const dlka_lka3d_params *p, void *y,
                                        void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                                        int B, int C, int D, int H, int W, int dtype, void *stream);
/* Weight preparation of MANY blocks in ONE launch.  The forward call above re-lays the block's weights into MFMA operand order (12 small
 * jobs, one launch per block; inside a hipGraph every dependent node costs ~4.5 us, and at C = 256 the launch itself is 41 us).  The prepared
 * forms depend on the parameters only, so a model that steps all its blocks (the 21 blocks of a D_LKA_Former patch) prepares them together,
 * once per optimizer step:
 *   plan_bytes  size of the job table;  _prepare_plan fills a HOST buffer (pointers of every block's parameters and `saved` area; they must stay
 *   put); the caller copies it to the device once;  _prepare_run(plan_device, plan_host, n) = one launch;  _forward_prepared = the forward call
 *   without its preparation launch.  params: array of n structs; dims5: n x (B, C, D, H, W). */
size_t dlka_lka3d_tokens_prepare_plan_bytes(int nblocks);
int dlka_lka3d_tokens_prepare_plan(int nblocks, const dlka_lka3d_params *params, void *const *saved, const size_t *saved_bytes,
                                   const int *dims5, int dtype, void *plan_host, size_t plan_bytes);
int dlka_lka3d_tokens_prepare_run(const void *plan_device, const void *plan_host, int nblocks, void *stream);
/* the same for blocks [block_lo, block_hi) only: a caller can prepare the first blocks, start their forward passes, and prepare the rest on another stream */
int dlka_lka3d_tokens_prepare_run_range(const void *plan_device, const void *plan_host, int nblocks, int block_lo, int block_hi, void *stream);
int dlka_lka3d_attention_tokens_forward_prepared(const void *x, const dlka_lka3d_params *p, void *y,
                                                 void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                                                 int B, int C, int D, int H, int W, int dtype, void *stream);
int dlka_lka3d_attention_tokens_backward(const void *x, const dlka_lka3d_params *p, const void *grad_y,
                                         const void *saved, size_t saved_bytes,
                                         void *grad_x, const dlka_lka3d_grads *grads,
                                         void *workspace, size_t workspace_bytes,
                                         int B, int C, int D, int H, int W, int dtype, void *stream);
/* Weight-gradient finalisation of MANY blocks in ONE launch.  The backward call above ends the block's seven weight gradients with one
 * "finalize" launch (fold of the row-chunk partial sums, re-layout of the depthwise staging): 21 dependent launches of 15 - 30 us per step for the
 * blocks of a D_LKA_Former patch, most of each latency.  Nothing later in the backward pass reads their results, so a model that steps all its
 * blocks lets the partial sums of every block land in a block-PRIVATE area and folds them all at the end of the pass (or of a slice of it):
 *   _partials_bytes_v        size of a block's private partial-sum area (one tile set per WORKGROUP of the weight-gradient kernels; DLKA_WGRAD_WAVES=1,
 *                            read per call, keeps one-wave workgroups and their larger areas: query and launch under the same setting — a launch that
 *                            finds the area too small returns DLKA_ERR_WORKSPACE);
 *   _plan_bytes / _plan_init a HOST job table for n blocks;
 *   _backward_deferred_v     the backward call without its finalize launch; partial sums go to `partials`; with plan_host != NULL it records the
 *                            block's jobs in slot `plan_slot` (pointers of `partials` and of the gradient buffers: they must stay put);
 *   _run_slot                (before sealing) finalises ONE recorded block with the ordinary per-block launch — what a caller does while the table is
 *                            still being recorded, e.g. when its first backward pass covers only a slice of the blocks;
 *   _plan_seal               after every slot has been recorded once: computes the launch geometry; the caller then copies the table to the device;
 *   _run(plan_device, plan_host, block_lo, block_hi)   ONE launch that finalises the weight gradients of blocks [block_lo, block_hi).
 * Results are identical to the per-block launch (same folds in the same order). */
size_t dlka_lka3d_tokens_partials_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant);
size_t dlka_wgrad_finalize_plan_bytes(int nblocks);
int dlka_wgrad_finalize_plan_init(void *plan_host, size_t plan_bytes, int nblocks);
int dlka_lka3d_attention_tokens_backward_deferred_v(const void *x, const dlka_lka3d_params *p, const void *grad_y,
                                                    const void *saved, size_t saved_bytes,
                                                    void *grad_x, const dlka_lka3d_grads *grads,
                                                    void *workspace, size_t workspace_bytes,
                                                    void *partials, size_t partials_bytes, void *plan_host, int plan_slot,
                                                    int B, int C, int D, int H, int W, int dtype, int variant, void *stream);
/* The deferred backward pass in two calls: phase 1 = the data-gradient chain (produces grad_x and, in `workspace`, everything the weight gradients
 * read), phase 2 = the five weight-gradient launches (reads them; records the block's finalize jobs).  Phase 2 may run on ANOTHER stream, after an
 * event recorded behind phase 1, so that it overlaps the next block's data chain — the caller then alternates two workspaces and makes phase 1 of a
 * block wait for the phase 2 that last used its workspace.  Same results as the one-call form. */
int dlka_lka3d_attention_tokens_backward_phase_v(const void *x, const dlka_lka3d_params *p, const void *grad_y,
                                                 const void *saved, size_t saved_bytes,
                                                 void *grad_x, const dlka_lka3d_grads *grads,
                                                 void *workspace, size_t workspace_bytes,
                                                 void *partials, size_t partials_bytes, void *plan_host, int plan_slot, int phase,
                                                 int B, int C, int D, int H, int W, int dtype, int variant, void *stream);
int dlka_wgrad_finalize_run_slot(const void *plan_host, int plan_slot, void *stream);
int dlka_wgrad_finalize_plan_seal(void *plan_host);
int dlka_wgrad_finalize_run(const void *plan_device, const void *plan_host, int block_lo, int block_hi, void *stream);

/* =======================================================================================
 * TransformerBlock_3D_single_deform_LKA: what surrounds the D-LKA block
 * ======================================================================================= *
 * The reference wrapper (3D/d_lka_former/network_architecture/synapse/transformerblock.py:617-630) reshapes the NCDHW
 * volume to tokens (a permute copy), adds pos_embed, applies nn.LayerNorm, computes x + gamma * epa_block(...), permutes
 * back (another copy) and runs UnetResBlock (two 3^3 convs, BatchNorm3d, LeakyReLU 0.01; dynunet_block.py:12-80) and
 * Dropout3d + 1x1x1 conv.  Here everything stays in token / channels-last layout [M = B*N][C], fp32, C <= 256; the
 * convolutions go through dlka_conv3d_*_cl, the rest through the entry points below.                                  */

/* xt = tokens(x) (+ pos[N][C]);  xn = LayerNorm(xt) * w + b (biased variance, eps inside the sqrt: nn.LayerNorm, :609,:624);
 * stats[m] = {mean, rstd}.  x is the block input either as the NCDHW tensor itself (x_planar = 1: [B][C][N], read strided —
 * replaces the reshape/permute copy of :620) or already as tokens (x_planar = 0). */
int dlka_layernorm_tokens_forward(const void *x, int x_planar, const void *pos, const void *w, const void *b, void *xt, void *xn,
                                  void *stats, int B, int N, int C, float eps, int dtype, void *stream);
/* gxt = (g_res ? g_res : 0) + LayerNorm backward of g_xn;  gw, gb, gpos ([N][C], optional) fully overwritten. */
int dlka_layernorm_tokens_backward(const void *g_xn, const void *g_res, const void *xt, const void *stats, const void *w, void *gxt,
                                   void *gw, void *gb, void *gpos, int B, int N, int C, int dtype, void *stream);
/* out = xt + gamma[c] * e   (:624, gamma = 1e-6 * ones at construction, :610) */
int dlka_scale_residual_forward(const void *xt, const void *e, const void *gamma, void *out, int64_t M, int C, int dtype, void *stream);
/* ge = gamma[c] * g;  ggamma[c] = sum_m g * e */
int dlka_scale_residual_backward(const void *g, const void *e, const void *gamma, void *ge, void *ggamma, int64_t M, int C, int dtype,
                                 void *stream);
/* y = LeakyReLU(BatchNorm(x) (+ res))   (dynunet_block.py:68-79; nn.BatchNorm3d over (B, spatial) per channel).
 * training = 1: batch statistics are computed and written to stats = {mean[C], rstd[C], unbiased var[C]};
 * training = 0: stats[0..2C) = {running_mean, 1/sqrt(running_var + eps)} supplied by the caller.  scratch: 2*C floats. */
int dlka_batchnorm_cl_forward(const void *x, const void *res, const void *w, const void *b, void *stats, int training, void *y,
                              void *scratch, int64_t M, int C, float eps, float slope, int dtype, void *stream);
/* gx, gw, gb fully overwritten; gres (optional) = gradient of the residual input.  scratch: 2*C floats. */
int dlka_batchnorm_cl_backward(const void *g, const void *x, const void *y, const void *w, const void *stats, int training, void *gx,
                               void *gres, void *gw, void *gb, void *scratch, int64_t M, int C, float slope, int dtype, void *stream);
/* y[b][n][c] = x[b][n][c] * mask[b][c]   (nn.Dropout3d drops whole channels per sample, :611; the mask comes from the caller's RNG) */
int dlka_channel_scale(const void *x, const void *mask, void *y, int B, int64_t N, int C, int dtype, void *stream);

/* ---- planar (NCDHW) plumbing of the full D_LKA_Former --------------------------------------------------------------
 * nn.BatchNorm3d in TRAINING mode over fp32 [B][C][N] tensors (the UnetResBlock norms of encoder1 / decoder2 at full resolution,
 * 3D/d_lka_former/network_architecture/dynunet_block.py:66-80): y = (x - mean) rstd w + b with batch statistics;
 * stats = {mean[C], rstd[C], unbiased var[C], mean - pivot[C], pivot[C]} — 5*C floats, written by forward and read by backward; the pivot is the value the
 * sums are centred on, the median of five values of the channel's first plane; the caller updates its running estimates from rows 0 and 2;
 * w / b may be NULL; scratch: 2*C floats.
 * backward: gx fully overwritten, gw / gb (optional) = the affine gradients. */
int dlka_batchnorm_planar_forward(const void *x, const void *w, const void *b, void *stats, void *y, void *scratch,
                                  int B, int C, int64_t N, float eps, void *stream);
int dlka_batchnorm_planar_backward(const void *g, const void *x, const void *w, const void *stats, void *gx, void *gw, void *gb,
                                   void *scratch, int B, int C, int64_t N, void *stream);
/* 1x1x1 nn.Conv3d on fp32 planar tensors with few channels (the output heads, d_lka_former_synapse.py:148-150; conv3 of a UnetResBlock whose channel
 * count changes): y[b][co][v] = sum_ci W[co][ci] x[b][ci][v] + bias[co].  N % 4 == 0, Cin in {1, 2, 4, 8, 14, 16, 32}, Cout <= 64 (weight gradient:
 * Cout <= 16); anything else returns DLKA_ERR_UNSUPPORTED.  backward: gx / gw (+ gb) optional, fully overwritten. */
int dlka_pointwise_planar_forward(const void *x, const void *w, const void *bias, void *y, int B, int Cin, int Cout, int64_t N, void *stream);
int dlka_pointwise_planar_backward(const void *x, const void *w, const void *g, void *gx, void *gw, void *gb,
                                   int B, int Cin, int Cout, int64_t N, void *stream);

/* ---- the whole wrapper block, one call per direction --------------------------------------------------------------- */
/* Parameters of TransformerBlock_3D_single_deform_LKA other than epa_block's (those travel as dlka_lka3d_params):
 * state_dict keys norm.*, gamma, pos_embed, conv51.conv{1,2}.conv.weight, conv51.norm{1,2}.*, conv8.1.* (:609-616). */
typedef struct dlka_tblock3d_params {
    const void *norm_w, *norm_b;                         /* [C]             nn.LayerNorm                                   */
    const void *gamma;                                   /* [C]                                                           */
    const void *pos_embed;                               /* [N][C] or NULL  (pos_embed=False)                             */
    const void *conv51_conv1_w, *conv51_conv2_w;         /* [C][C][3][3][3] UnetResBlock convs, no bias                   */
    const void *conv51_norm1_w, *conv51_norm1_b;         /* [C]             BatchNorm3d affine                            */
    const void *conv51_norm2_w, *conv51_norm2_b;         /* [C]                                                           */
    const void *conv8_w, *conv8_b;                       /* [C][C][1][1][1], [C]   conv8[1]                               */
} dlka_tblock3d_params;

typedef struct dlka_tblock3d_grads { /* same shapes; all fully overwritten; pos_embed NULL iff the parameter is */
    void *norm_w, *norm_b, *gamma, *pos_embed, *conv51_conv1_w, *conv51_conv2_w, *conv51_norm1_w, *conv51_norm1_b,
         *conv51_norm2_w, *conv51_norm2_b, *conv8_w, *conv8_b;
} dlka_tblock3d_grads;

int dlka_tblock3d_supported(int B, int C, int D, int H, int W, int dtype);   /* fp32, C in {32,64,128,256} */
size_t dlka_tblock3d_saved_bytes(int B, int C, int D, int H, int W, int dtype);
size_t dlka_tblock3d_workspace_bytes(int B, int C, int D, int H, int W, int dtype);
/* Replaces TransformerBlock_3D_single_deform_LKA.forward (transformerblock.py:617-630).
 *   x: the block input, NCDHW [B][C][N] (x_planar = 1) or already tokens [B][N][C] (x_planar = 0, e.g. the previous block's y);
 *   y: tokens [B][N][C] — the reference's (B, C, H, W, D) result is the permuted VIEW of this memory;
 *   drop_mask: [B][C] multipliers of conv8[0] = Dropout3d(0.1) drawn by the caller's RNG ({0, 1/(1-p)}), NULL = no dropout (eval);
 *   bn_stats: 6*C floats {mean1, rstd1, var1, mean2, rstd2, var2}: written in training mode (var = unbiased batch variance, for the
 *             caller's running-statistics update), read in eval mode (mean = running_mean, rstd = 1/sqrt(running_var + eps));
 *             must be handed unchanged to the matching backward call, like `saved`. */
int dlka_tblock3d_forward(const void *x, int x_planar, const dlka_tblock3d_params *p, const dlka_lka3d_params *lka,
                          const void *drop_mask, int training, void *bn_stats, void *y,
                          void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                          int B, int C, int D, int H, int W, float ln_eps, float bn_eps, int dtype, void *stream);
/* grad_y, grad_x: tokens [B][N][C] (grad wrt the NCDHW input is the permuted view of grad_x). */
int dlka_tblock3d_backward(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training,
                           const void *bn_stats, const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x,
                           const dlka_tblock3d_grads *grads, const dlka_lka3d_grads *lka_grads,
                           void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream);

/* 2-D counterpart (torchvision 0.12 deform_conv2d, un-vendored; 2D/deformable_LKA/deformable_LKA.py:18-30): idx int32 [B][og][K][No][2]
 * = the floor cell (y, x) where `reach`, else 0; mask uint8: bit 0 = the sample is inside the guard (-1 < q < size), bit 1 = reach
 * (q >= -1 && q < size: the domain of torchvision's unguarded coordinate weight).  path 0 = sample_cell2 (deform_sample.h; the
 * window scatter of cl_ddw2d.hip calls it directly), path 1 = setup_tap<2> (general kernels), path 2 = describe2 (cl_ddw2d.hip). */
int dlka_deform_conv2d_sample_index_path(const void *offset, int32_t *idx, uint8_t *mask,
                                         const dlka_conv_geom *g, int dtype, int path, void *stream);

/* Channels-last 2-D DEPTHWISE deformable conv on its own — the two large-kernel convs of the 2-D D-LKA block
 * (2D/deformable_LKA/deformable_LKA.py:93-94 -> :18-30: torchvision.ops.DeformConv2d(C, C, k, padding, groups=C, dilation,
 * bias=False)(x, offsets)).  x / out / grad_out / grad_x [B][H][W][C]; offset / grad_offset [B][2 kh kw][H][W] ((dy, dx) per tap, as
 * torchvision); weight / grad_weight [C][1][kh][kw].  Stride 1, "same" padding, C % 32 == 0, fp32.  All three gradients at once. */
size_t dlka_deform_dwconv2d_cl_workspace(const dlka_conv_geom *g, int dtype, int backward);
int dlka_deform_dwconv2d_forward_cl(const void *x, const void *offset, const void *weight, void *out,
                                    void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);
int dlka_deform_dwconv2d_backward_cl(const void *x, const void *offset, const void *weight, const void *grad_out,
                                     void *grad_x, void *grad_offset, void *grad_weight,
                                     void *workspace, size_t workspace_bytes, const dlka_conv_geom *g, int dtype, void *stream);

/* =======================================================================================
 * Net variants of the 3-D block (the depthwise pair conv0 / conv_spatial of LKA3d_deform)
 * =======================================================================================
 * DLKA_LKA3D_SYNAPSE  3D/d_lka_former/network_architecture/synapse/transformerblock.py:637-638 (and the pancreas copy): 5^3 pad 2, then
 *                     7^3 dilation 3 pad 9, at every width.  All entry points without the _v suffix.
 * DLKA_LKA3D_ACDC     3D/d_lka_former/network_architecture/acdc/transformerblock.py:213-237: C <= 64: 5^3 pad 2, (5,7,7) dilation 3 pad (6,9,9);
 *                     C = 128: 5^3 pad 2, (3,5,5) dilation (1,3,3) pad (1,6,6); C = 256: 3^3 pad 1, 3^3 pad 1 — the stem (1,4,4) net whose stage
 *                     shapes BASELINE.json config 5's 40x224x224 tiles divide through (acdc/model_components.py:21).  conv0_w / conv_spatial_w
 *                     (and their gradients) have the variant's kernel shapes.
 * The _v entry points are their un-suffixed namesakes with the variant as an extra argument (before `stream`). */
typedef enum dlka_lka3d_variant { DLKA_LKA3D_SYNAPSE = 0, DLKA_LKA3D_ACDC = 1 } dlka_lka3d_variant;
int    dlka_lka3d_tokens_supported_v(int B, int C, int D, int H, int W, int dtype, int variant);
size_t dlka_lka3d_tokens_saved_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant);
/* Forces (1) / releases (0) the deformable weight gradient that GATHERS for itself (no sample tensor handed over by the grad_offset kernel);
 * returns the previous setting.  Initial value: 1 iff the environment variable DLKA_WGRAD_GATHER is set when the first token-path call is made.
 * For A/B runs and the hand-over parity test; the workspace size query always covers both routes. */
int dlka_lka3d_force_wgrad_gather(int on);
/* Fork contexts.  Some backward entry points run independent kernels of ONE call on library-internal streams, forked from and
 * joined back into the caller's stream inside the call (dlka_lka2d_attention_backward; the data-chain pass of the block-stack engine).  The streams and
 * events of a call are a context leased from a per-DEVICE pool for the duration of that call: a call issued with device k current uses handles of device k
 * only (nn.DataParallel replicas, 2D/trainer_MaxViT_deform_LKA.py:107-108), two host threads inside the library at once hold different contexts, contexts
 * are never created inside a stream capture, and an error return joins what was forked.  dlka_fork_stats: contexts created on / leases handed out for
 * `device` so far in this process (tests: no handle of device 0 is touched by a call on device 1; two concurrent callers got two contexts).
 * dlka_env_refresh: the switches DLKA_GX_FORK_MIN_ROWS and DLKA_LKA2D_FORK are read once per process; this re-reads them (tests and A/B scripts that
 * change them in-process call it afterwards). */
int  dlka_fork_stats(int device, int64_t *contexts, int64_t *leases);
void dlka_env_refresh(void);
/* Diagnostics: launches so far (this process) of the opt-in LDS-brick depthwise kernel (csrc/cl_dwconv_lds.hip; DLKA_DW_LDS=1: the dw 5^3 / 7^3
 * dilation-3 convs of the block and their data gradients take it where the volume is large enough, =2: wherever its geometry fits; default: never —
 * it measured no faster than the register-row kernel); the tests use it to assert WHICH kernel produced the result they compare. */
long dlka_dwconv_lds_launch_count(void);
/* launches so far of the LDS-brick data gradient of the offset-predict conv (csrc/cl_conv_brick.hip): parity tests assert which kernel ran */
long dlka_conv_brick_launch_count(void);
/* launches so far of the fused small-volume depthwise pair (csrc/cl_dwpair.hip: dw 5^3 -> dw 7^3 dil 3, or their data gradients + GELU', of a volume of at most
 * 512 voxels with W in {4, 8} in ONE launch; DLKA_DWPAIR=0, read per call, keeps one launch per conv): parity tests assert which kernel ran */
long dlka_dwpair_launch_count(void);
/* launches so far of the workgroup-tiled pointwise chain (csrc/cl_pointwise.hip, cl_pointwise_chain_kernel: conv1 + gate -> proj_2 + shortcut, or their data
 * gradients, of a token-layout block with C = 64 / 128 in ONE launch, bit-identical to the two launches; C = 256 only with DLKA_PW_CHAIN_256=1: it measured slower; DLKA_PW_UNFUSED=1, read per call, keeps those):
 * parity tests assert which kernel ran */
long dlka_pw_chain_launch_count(void);
/* Diagnostics: launches of cl_conv_kw_kernel (round 6: the small-volume split-operand convs — offset-predict conv, its data gradient, UnetResBlock's 3^3 convs at the
 * 16^3 / 8^3 / 4^3 stages — with the contraction split over the waves of ONE workgroup and summed in wave order in LDS: bitwise reproducible, no global atomics;
 * DLKA_CONV_KW=0 restores the tap split over the grid) and of the deformable forward's workgroup-split variants.  Tests assert which kernel ran. */
long dlka_conv_kw_launch_count(void);
/* Diagnostics: would a conv of this form take cl_conv_kw_kernel (1) or not (0)?  amode: 0 channels-last input, 2 planar gradient input; omode: 0 channels-last, 1 planar
 * output; split_bf16: 0 exact fp32, 2 / 3 two- / three-term operands; K taps; epi: 0 none, 3 "+ aux"; NP: output columns padded to 32; volume: D > 1.  The planar store
 * has no aux add, so epi = 3 with omode = 1 is refused (tests/test_small_fixes.py). */
int dlka_conv_kw_applies(int amode, int omode, int split_bf16, int K, int epi, int NP, int act_bf16, int volume);
size_t dlka_lka3d_tokens_workspace_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant);
int dlka_lka3d_attention_tokens_forward_v(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t saved_bytes,
                                          void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant, void *stream);
int dlka_lka3d_attention_tokens_backward_v(const void *x, const dlka_lka3d_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                           void *grad_x, const dlka_lka3d_grads *grads, void *workspace, size_t workspace_bytes,
                                           int B, int C, int D, int H, int W, int dtype, int variant, void *stream);
int    dlka_tblock3d_supported_v(int B, int C, int D, int H, int W, int dtype, int variant);
/* dtype on the wrapper-block entry points: DLKA_F32, or DLKA_BF16 = MIXED precision — x, y, grad_y, grad_x, the residual stream, LayerNorm / BatchNorm
 * statistics, the 3^3 convs of UnetResBlock and all parameter gradients stay fp32 (the pointers are fp32 tensors on both dtypes); the D-LKA attention
 * inside (transformerblock.py:624) runs DLKA_BF16: its input, output and their gradients are bf16 storage, with the token path's rule (the chain that
 * decides the sampling cells fp32, fp32 parameters / offsets / accumulation).  What torch.autocast(bfloat16) selects for the module. */
size_t dlka_tblock3d_saved_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant);
/* Diagnostics (bench health check, the parity tests' cell-flip analysis): byte offset, inside the opaque `saved` buffer of a token-layout
 * forward call / of a wrapper-block forward call, of the predicted sampling offsets [B][81][D][H][W] (fp32 on both dtypes, the reference's planar
 * layout, deform_im2col_cuda.cuh:237-243). */
int dlka_lka3d_tokens_saved_offsets_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t *byte_offset);
int dlka_tblock3d_saved_offsets_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t *byte_offset);
/* Diagnostics (the parity tests' LeakyReLU-kink analysis): byte offsets, inside the `saved` buffer of a wrapper-block forward call, of the two tensors
 * whose SIGN is the activation pattern of UnetResBlock's two LeakyReLUs (dynunet_block.py:69-70,77-79): byte_offsets[0] = a1 = lrelu(norm1(conv1(x))),
 * byte_offsets[1] = rd = dropout3d(lrelu(norm2(conv2(a1)) + x)); both fp32 tokens [B][N][C] on both dtypes. */
int dlka_tblock3d_saved_activations_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t byte_offsets[2]);
size_t dlka_tblock3d_workspace_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant);
int dlka_tblock3d_forward_v(const void *x, int x_planar, const dlka_tblock3d_params *p, const dlka_lka3d_params *lka,
                            const void *drop_mask, int training, void *bn_stats, void *y, void *saved, size_t saved_bytes,
                            void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, float ln_eps, float bn_eps,
                            int dtype, int variant, void *stream);
int dlka_tblock3d_backward_v(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training,
                             const void *bn_stats, const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x,
                             const dlka_tblock3d_grads *grads, const dlka_lka3d_grads *lka_grads,
                             void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant, void *stream);
/* The same pass in two parts (phase 0 = dlka_tblock3d_backward_v).  phase 1: the DATA-gradient chain — grad_x and the gradients its own kernels produce (norm / norm1 /
 * norm2 affine parameters, gamma, pos_embed) —, leaving in `workspace` what phase 2 reads; phase 2: the weight gradients of conv51.conv1 / conv2, conv8 and of the D-LKA
 * attention, and the fold of their partial sums.  Issue phase 2 on another stream behind an event recorded after phase 1 (same arguments; `workspace` untouched in
 * between) and a block's weight gradients overlap the next block's data chain (deformablelka_amd/transformerblock.py: wgrad_overlap). */
int dlka_tblock3d_backward_phase_v(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training, const void *bn_stats,
                                   const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x, const dlka_tblock3d_grads *grads,
                                   const dlka_lka3d_grads *lka_grads, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype,
                                   int variant, int phase, void *stream);

/* =======================================================================================
 * Sliding-window prediction with test-time mirroring — csrc/cl_tiles.hip
 * =======================================================================================
 * nnU-Net's SegmentationNetwork._internal_predict_3D_3Dconv_tiled (3D/d_lka_former/network_architecture/neural_network.py:292-428)
 * with _internal_maybe_mirror_and_pred_3D (:502-560): per tile the patch and its flips go through the net, the nonlinearity's
 * outputs are flipped back and averaged, multiplied by the Gaussian importance map and added into the score map.  Here a CHUNK of
 * T tiles and its M mirrors is one network batch [T*M] (tile-major: b = t*M + m), produced by dlka_tiles_gather and consumed by
 * dlka_tiles_blend; dlka_tiles_finalize runs once at the end.
 *
 *   origins  HOST int[T][3]: the tiles' low corners (x, y, z) in PADDED coordinates, in the reference's step order (:374-380)
 *   masks    HOST int[M]: mirror masks, bit 0 = flip x, bit 1 = flip y, bit 2 = flip z, in the order the reference visits them
 *            (m = 0..7 at :526-557 is the mask {0, z, y, yz, x, xz, xy, xyz} filtered by mirror_axes)
 *   patch    pd x ph x pw; volumes x (C, X, Y, Z), score map [K][Xp][Yp][Zp] fp32, weight map [Xp][Yp][Zp] fp32, contiguous
 *
 * Addition order (dlka_tiles_blend; bitwise that of the reference's sequential loops, :403-415 and :526-559):
 *   for each voxel, for t = 0 .. T-1 among the tiles covering it:
 *       r_k  = 0;  for m in masks order: r_k = r_k + mirror_scale * nonlin(logits)[t*M + m][k][flip_m(voxel - origin_t)]
 *       r_k  = r_k * g[voxel - origin_t]          (g = 1 without importance map)
 *       score_k = score_k + r_k;  weight = weight + g
 * Every product and sum is rounded on its own (no FMA contraction); no atomics: two calls give identical bits.  mirror_scale is
 * 1 / 2^len(mirror_axes) (:517-518).  Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (non-positive size; a tile outside the score map;
 * a kept region outside it), DLKA_ERR_UNSUPPORTED (T > DLKA_TILES_MAX_T, M > 8, a mask outside 0..7, K > DLKA_TILES_K_MAX or an
 * unknown nonlinearity: nothing is launched), DLKA_ERR_DTYPE. */
#define DLKA_TILES_MAX_T 64      /* tiles per chunk */
#define DLKA_TILES_K_MAX 32      /* classes the blend keeps in registers (Synapse 14, ACDC 4) */
#define DLKA_TILES_IDENTITY 0    /* nonlinearity codes of dlka_tiles_blend: inference_apply_nonlin = identity (neural_network.py SegmentationNetwork default) */
#define DLKA_TILES_SOFTMAX 1     /*   softmax over the K classes (softmax_helper, d_lka_former_trainer_synapse.py:185) */
#define DLKA_TILES_SIGMOID 2     /*   elementwise sigmoid */
/* out [T*M][C][pd][ph][pw] fp32 = torch.flip(pad(x)[:, o:o+p], flipped axes of mask m) for b = t*M + m.  x is the UNPADDED volume
 * (C, X, Y, Z); pad_x/y/z = the low-side constant padding of pad_nd_image(..., 'constant') (d // 2); a read outside x gives
 * pad_value (pad_kwargs['constant_values']).  A pure copy (bitwise). */
int dlka_tiles_gather(const float *x, int C, int X, int Y, int Z, const int *origins, int T, const int *masks, int M, int pd, int ph,
                      int pw, int pad_x, int pad_y, int pad_z, float pad_value, float *out, void *stream);
/* score / weight += the chunk's blended prediction (order above).  logits [T*M][K][pd][ph][pw], dtype DLKA_F32 or DLKA_BF16 (the net
 * under bf16 autocast; arithmetic fp32); nonlin DLKA_TILES_*; gauss [pd][ph][pw] fp32 or NULL. */
int dlka_tiles_blend(const void *logits, int dtype, int K, int nonlin, float mirror_scale, const float *gauss, float *score,
                     float *weight, int Xp, int Yp, int Zp, const int *origins, int T, const int *masks, int M, int pd, int ph, int pw,
                     void *stream);
/* The kept region [pad, pad + (X, Y, Z)) (:420-428): probs [K][X][Y][Z] fp32 = score / weight, seg [X][Y][Z] int64 = the index of the
 * first maximum over K (torch.argmax: a NaN counts as the maximum). */
int dlka_tiles_finalize(const float *score, const float *weight, int K, int Xp, int Yp, int Zp, int pad_x, int pad_y, int pad_z, int X,
                        int Y, int Z, float *probs, int64_t *seg, void *stream);
/* Diagnostics: launches so far (this process) of the three kernels above; the tests assert that the HIP path ran. */
long dlka_tiles_launch_count(void);

/* =======================================================================================
 * Segmentation losses of the two trainers — csrc/cl_seg_loss.hip
 * =======================================================================================
 * The 3-D trainer steps nnU-Net's DC_and_CE_loss({'batch_dice': True, 'smooth': 1e-5, 'do_bg': False}, {})
 * (3D/d_lka_former/training/network_training/Trainer_synapse.py:109; loss_functions/dice_loss.py:158-194 SoftDiceLoss, :304-361
 * DC_and_CE_loss, :100-155 get_tp_fp_fn_tn) per deep-supervision head; the 2-D trainer steps 0.4 CE + 0.6 DiceLoss(softmax=True)
 * (2D/trainer_MaxViT_deform_LKA.py:137-139; 2D/utils.py:11-47).  Both are functions of per-(sample, class) sums over the voxels of
 * p = softmax(logits, 1):
 *      tp = sum p_k [y = k]     sp = sum p_k     sq = sum p_k^2     cnt = sum [y = k]     and per sample  ce = sum (logsumexp - x_y)
 * (nnU-Net's fp = sp - tp and fn = cnt - tp, so 2 tp + fp + fn = sp + cnt).
 *
 *   logits   planar [B][K][N], N = product of the spatial extents (rank 4 and rank 5 alike), DLKA_F32 or DLKA_BF16, contiguous
 *   labels   [B][N] label map, DLKA_LABEL_F32 (what both reference loaders deliver) or DLKA_LABEL_I64, read as they are
 *
 * mode DLKA_SEG_LOSS_NNUNET:   dc = (2 tp + smooth) / (sp + cnt + smooth + 1e-8) per (b, k), or per k with the sums taken over the batch
 *                              (batch_dice); class 0 dropped unless do_bg;  loss = weight_ce * mean_voxels(ce) - weight_dice * mean(dc)
 * mode DLKA_SEG_LOSS_DICE2D:   dice_k = 1 - (2 sum_b tp + 1e-5) / (sum_b sq + sum_b cnt + 1e-5);  loss = sum_k class_weight[k] dice_k / K
 *                              (smooth, weight_*, batch_dice, do_bg are not read)
 *
 * A label that is not an integer in [0, K) never indexes anything: it belongs to no class.  In NNUNET mode (the reference's scatter_
 * would raise) the loss and the gradient are NaN; in DICE2D mode (one-hot by equality, utils.py:16-22) that is the reference's result.
 *
 * forward: one streaming launch (one partial row per workgroup in `workspace`) and one finishing launch that adds the rows in a fixed
 * order in double precision: no atomics, no host read, bitwise reproducible, capturable.  Outputs (device, fp32):
 *   loss[1];  dc[B][K] (NNUNET: the Dice coefficients, all rows equal under batch_dice, 0 for a dropped background; DICE2D: 1 - dice_k);
 *   stats[B][4K + 2] = tp[K], sp[K], sq[K], cnt[K], ce, number of invalid labels;
 *   coef[B][3][K] + 1: the backward's per-class scalars, dloss/dp_k(v) = coef[b][0][k] + coef[b][1][k] p_k + coef[b][2][k] [y(v) = k], then
 *   the cross-entropy scale weight_ce / (B N).
 * backward: one streaming launch; recomputes the softmax, grad_logits_j = grad_output * (p_j (g_j - sum_k g_k p_k) + ce_scale (p_j - [y = j])),
 * written once in the logits' dtype.  grad_output: one fp32 value in device memory.
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE, DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (K > DLKA_SEG_LOSS_K_MAX, unknown mode),
 * DLKA_ERR_WORKSPACE. */
#define DLKA_SEG_LOSS_K_MAX 32
#define DLKA_SEG_LOSS_NNUNET 0
#define DLKA_SEG_LOSS_DICE2D 1
#define DLKA_LABEL_F32 0
#define DLKA_LABEL_I64 1
typedef struct dlka_seg_loss_desc {
    int32_t B, K;
    int64_t N;
    int32_t dtype, label_dtype, mode, batch_dice, do_bg;
    float smooth, weight_ce, weight_dice;
    float class_weight[DLKA_SEG_LOSS_K_MAX];   /* DICE2D: `weight` of DiceLoss.forward (utils.py:37-38: ones when absent) */
} dlka_seg_loss_desc;
/* bytes of `workspace` for dlka_seg_loss_forward and dlka_seg_eval_counts of this shape (0 for an invalid description) */
size_t dlka_seg_loss_workspace_bytes(const dlka_seg_loss_desc *d);
int dlka_seg_loss_forward(const void *logits, const void *labels, const dlka_seg_loss_desc *d, void *workspace, size_t workspace_bytes,
                          float *loss, float *dc, float *stats, float *coef, void *stream);
int dlka_seg_loss_backward(const void *logits, const void *labels, const dlka_seg_loss_desc *d, const float *coef, const float *grad_output,
                           void *grad_logits, void *stream);
/* Trainer_synapse.py:697-718 (run_online_evaluation) without its softmax and masked passes: seg = first-maximum argmax of the logits
 * (torch.argmax; softmax is monotonic), counts[3][K - 1] int64 = hard tp / fp / fn of the foreground classes 1 .. K-1, summed over the
 * batch.  Reads B, K, N and the two dtypes of `d`.  Two launches (stream + finish), integer arithmetic throughout. */
int dlka_seg_eval_counts(const void *logits, const void *labels, const dlka_seg_loss_desc *d, void *workspace, size_t workspace_bytes,
                         int64_t *counts, void *stream);
/* Diagnostics: kernel launches so far (this process) of the three entries above. */
long dlka_seg_loss_launch_count(void);

/* =======================================================================================
 * Overlap counts and surface distances of label maps (DSC, HD, HD95, ASD) — csrc/cl_surface_dist.hip
 * =======================================================================================
 * Every evaluator of the reference scores a prediction with medpy.metric.binary.dc and hd95 on whole volumes, per organ
 * (2D/utils.py:50-60 calculate_metric_percase, :96-98 test_single_volume; 3D/d_lka_former/inference_synapse.py:11-21;
 * inference_acdc.py:29-51; 3D/pancreas_code/test_util.py:130; 3D/d_lka_former/evaluation/metrics.py:314-383 hausdorff_distance,
 * hausdorff_distance_95, avg_surface_distance, avg_surface_distance_symmetric).  MedPy 0.4.0:
 *      border(m) = m ^ binary_erosion(m, generate_binary_structure(rank, connectivity))       (cells outside the array count as 0)
 *      sds(a, b) = distance_transform_edt(~border(b), sampling = spacing)[border(a)]
 * and dc = 2 |a & b| / (|a| + |b|), hd = max, hd95 = 95th percentile of sds(a, b) ++ sds(b, a), asd = mean of sds(a, b).
 *
 *   prediction, label   two maps of equal extents ext[3] = (d, h, w), w contiguous; rank 2 has ext[0] = 1 (and no neighbours along d: a
 *                       rank-3 map of depth 1 is all border).  Same dtype, DLKA_SD_U8 (bool too) / I16 / I32 / I64, read as they are.
 *   classes             class_id[K]: mask_c = (map == class_id[c]).  mask_mode != 0: K = 1 and mask = (map != 0), medpy's astype(bool).
 *
 * dlka_sd_label_stats: stats[K][9] int64 (device) = |a & b|, |a|, |b|, then lo d h w and hi d h w of the bounding box of a | b (lo > hi when
 * the class is absent from both maps).  One pass over both maps per 4 classes and one finishing launch; integers, fixed order.
 *
 * dlka_sd_distances: boxes[K][6] int64 (HOST) = lo d h w, extent d h w of the region to transform for each class, inside the array; an
 * extent of 0 skips the class.  The box must contain both masks of its class (the box of the stats above does; so does the whole array):
 * then the result equals that of the whole array, because outside the box both masks are 0 just as outside the array.  For class c with
 * n_c box cells, sqdist[off_c .. off_c + n_c) holds, in box order, the SQUARED Euclidean distance sum_i (delta_i spacing_i)^2 (float64;
 * with unit spacing an exact integer) from each border cell of the prediction's mask to the nearest border cell of the label's, and -1 at
 * every other cell; sqdist[off_c + n_c .. off_c + 2 n_c) the same from the label's border to the prediction's.  off_c = sum of 2 n_j over
 * the classes before c; dlka_sd_distance_cells returns the total (-1 for an invalid description or box).  Exact: every candidate of every
 * line is visited.  No atomics: bitwise reproducible.  workspace: 12 bytes per cell of the total.
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (rank not 2 or 3, extents, spacing not positive, a box outside the array, sqdist too short),
 * DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (connectivity outside 1..rank, K outside 1..DLKA_SD_K_MAX, more than 2^31 - 1 cells, w > 32768),
 * DLKA_ERR_WORKSPACE.  Nothing is read before the checks pass. */
#define DLKA_SD_K_MAX 32
#define DLKA_SD_U8 0
#define DLKA_SD_I16 1
#define DLKA_SD_I32 2
#define DLKA_SD_I64 3
typedef struct dlka_sd_desc {
    int32_t rank, connectivity, label_dtype, K, mask_mode;
    int64_t ext[3];
    double spacing[3];                    /* per axis d, h, w (rank 2: [0] is not read); None of medpy = 1.0 */
    int64_t class_id[DLKA_SD_K_MAX];
} dlka_sd_desc;
size_t dlka_sd_stats_workspace_bytes(const dlka_sd_desc *d);   /* 0 for an invalid description */
/* dc's three counts per class (medpy.metric.binary.dc; inference_synapse.py:11-21) and the crop box of the transform */
int dlka_sd_label_stats(const void *prediction, const void *label, const dlka_sd_desc *d, void *workspace, size_t workspace_bytes,
                        int64_t *stats, void *stream);
int64_t dlka_sd_distance_cells(const dlka_sd_desc *d, const int64_t *boxes);
/* medpy.metric.binary.__surface_distances for every class and both directions (hd, hd95, asd, assd; metrics.py:314-383) */
int dlka_sd_distances(const void *prediction, const void *label, const dlka_sd_desc *d, const int64_t *boxes, void *workspace,
                      size_t workspace_bytes, double *sqdist, int64_t sqdist_cells, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_sd_launch_count(void);

/* =======================================================================================
 * Connected components of label maps and the "largest component" filter — csrc/cl_conn_comp.hip
 * =======================================================================================
 * nnU-Net's post-processing as the reference runs it at the end of Trainer_synapse.validate() / Trainer_acdc.validate()
 * (determine_postprocessing) and for every predicted case in inference/predict.py (load_remove_save):
 * remove_all_but_the_largest_connected_component, 3D/d_lka_former/postprocessing/connected_components.py:48-105 — per class or region
 * one scipy.ndimage.label (:76), object sizes (:80-81), the largest object and every object of its size kept (:89-94), the others removed
 * when no minimum size is given or when they are smaller than it (:96-100), the largest removed size recorded (:101-104).
 *
 *   image               one map of rank 1..3, extents left-padded with 1 to ext[3] = (d, h, w), w contiguous; DLKA_SD_U8 (bool too) / I16 / I32 / I64.
 *   entries             K entries, each a set of class ids: class_id[j] belongs to entry entry_of[j], j < n_ids; the ids are pairwise different
 *                       (a cell belongs to at most one entry).  mask_mode != 0: K = 1, the entry is (image != 0), scipy.ndimage.label's input.
 *   neighbourhood       generate_binary_structure(rank, connectivity), connectivity 1..rank; cells outside the array are background.  Two
 *                       neighbouring cells are connected iff they belong to the same entry.
 *   filter              a component is kept when its size equals its entry's largest, or when has_min != 0 and its size >= min_count[entry]
 *                       (cells; the caller turns the reference's float threshold into the count that compares alike).
 *
 * dlka_cc_components: labels[N] int32 = 0 for background, else 1 + the number of components whose first cell comes earlier in raster order
 * (scipy's numbering, over all entries of the pass together); filtered[N] (dtype of the image; may be NULL, must not be the image) = the image
 * with the removed components set to 0; summary[DLKA_CC_SUMMARY] int32 (device) = [0] the number of components, [1 + e] the largest size of
 * entry e (0: no cell), [1 + DLKA_CC_K_MAX + e] the largest removed size of entry e (0: nothing removed).  Six launches and one memset on
 * `stream`; integer atomics only, every output bitwise reproducible (the argument is in the file's header).
 * dlka_cc_component_table: after dlka_cc_components with the same description and workspace (untouched in between): sizes[capacity] int64 and
 * owner[capacity] int32 (the entry) of component r + 1 at index r; components beyond `capacity` are not written.  One launch.
 * workspace: 9 bytes per cell plus 4 per 2048 cells (dlka_cc_workspace_bytes; 0 for an invalid description).
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (rank outside 1..3, an extent < 1, a padded extent != 1, entry_of outside 0..K-1, a negative
 * min_count or capacity), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (connectivity outside 1..rank, K outside 1..DLKA_CC_K_MAX, n_ids outside
 * 1..DLKA_CC_IDS_MAX, an id listed twice, 2^31 cells or more, filtered == image), DLKA_ERR_WORKSPACE.  Nothing is launched before the
 * checks pass.  The contiguous axis has no limit of its own: a line longer than a tile (64 cells; 2048 for a single line) spans tiles. */
#define DLKA_CC_K_MAX 32
#define DLKA_CC_IDS_MAX 64
#define DLKA_CC_SUMMARY (1 + 2 * DLKA_CC_K_MAX)
typedef struct dlka_cc_desc {
    int32_t rank, connectivity, label_dtype, K, mask_mode, n_ids, has_min;
    int64_t ext[3];
    int64_t class_id[DLKA_CC_IDS_MAX];
    int32_t entry_of[DLKA_CC_IDS_MAX];
    int64_t min_count[DLKA_CC_K_MAX];
} dlka_cc_desc;
size_t dlka_cc_workspace_bytes(const dlka_cc_desc *d);
int dlka_cc_components(const void *image, const dlka_cc_desc *d, void *workspace, size_t workspace_bytes, int32_t *labels, void *filtered,
                       int32_t *summary, void *stream);
int dlka_cc_component_table(const dlka_cc_desc *d, const void *workspace, size_t workspace_bytes, int64_t capacity, int64_t *sizes,
                            int32_t *owner, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_cc_launch_count(void);

/* =======================================================================================
 * Resampling of probabilities, images and label maps; resampling fused with the argmax — csrc/cl_resample.hip
 * =======================================================================================
 * resample_data_or_seg (3D/d_lka_former/preprocessing/preprocessing.py:112-201) as save_segmentation_nifti_from_softmax calls it for the class
 * probabilities (inference/segmentation_export.py:104-106, followed by the argmax of :119-125) and resample_patient for a case and its label
 * map (preprocessing.py:99-108).  skimage's resize(mode='edge', anti_aliasing=False), batchgenerators' resize_segmentation and the
 * reference's own z step (:163-187) all sample the source at (i + 0.5) * n_in / n_out - 0.5 per axis.
 *
 *   volumes     C channels of extents in[3], the last axis contiguous, channels in_cells apart; results out[3] likewise.
 *   tables      built by the caller in float64, on the device, the three axes one after the other (axis ax starts at row out[0] + .. +
 *               out[ax - 1]).  Linear entries: idx[2 * row + k] (source cell, 0 <= idx < in[ax]) and w[2 * row + k], k < 2; an axis with
 *               taps[ax] == 1 reads k = 0 only (order 0: the nearest cell, weight 1).  Spline entries: start[row], w4[4 * row + k];
 *               taps[ax] is 4 (cells start .. start + 3 of the coefficient array) or 1.  The library cannot check the cells a table names.
 *
 * dlka_resample_argmax (:104-106 and :119-125 in one pass): labels[out cells] uint8 = the first maximum over the C resampled channels
 * (numpy.argmax), or with region_class (C values, device) the value of the last channel whose resampled value is > 0.5, else 0.  The
 * resampled channels are never stored.  dlka_resample_linear (:153-158, :177, :196 for orders 0 and 1): every channel stored; the same
 * arithmetic in the same order, so the argmax of its output is dlka_resample_argmax's map bit for bit.  dtype: DLKA_F32 or DLKA_F64.
 * dlka_resample_labels (resize_segmentation as :127, :153-158, :196 bind it; strict != 0: the z step of :180-187): int32 maps; per output cell
 * the largest label whose summed weight is >= 0.5 (strict: > 0.5) among the source cells, 0 when there is none.
 * dlka_resample_spline_eval (order 3, :130-131 with :153-158 or :196): float64; the 4-tap evaluation of one channel of B-spline coefficients
 * (dlka_spline_pad with DLKA_RESAMPLE_SPLINE_PAD edge samples on every filtered axis, dlka_spline_prefilter with DLKA_SPLINE_REFLECT along
 * it) clipped to [lo[s], hi[s]], s = the output index along clip_axis, or 0 when clip_axis < 0.
 * One launch each, no atomics: results are bitwise reproducible.  Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (C or an extent < 1, a clip
 * axis above 2), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (taps other than 1 or 2 (spline: 4), 2^31 cells or more, C > 256 for the argmax,
 * C != 1 for the spline, output == input).  Nothing is launched before the checks pass. */
typedef struct dlka_resample_desc {
    int32_t C, dtype;
    int32_t taps[3];
    int64_t in[3], out[3];
} dlka_resample_desc;
int dlka_resample_argmax(const void *x, uint8_t *labels, const dlka_resample_desc *d, const int32_t *idx, const double *w,
                         const int32_t *region_class, void *stream);
int dlka_resample_linear(const void *x, void *y, const dlka_resample_desc *d, const int32_t *idx, const double *w, void *stream);
int dlka_resample_labels(const int32_t *seg, int32_t *out, const dlka_resample_desc *d, const int32_t *idx, const double *w, int strict,
                         void *stream);
int dlka_resample_spline_eval(const double *coef, double *y, const dlka_resample_desc *d, const int32_t *start, const double *w4,
                              const double *lo, const double *hi, int clip_axis, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above and of dlka_spline_pad / dlka_spline_prefilter below. */
long dlka_resample_launch_count(void);

/* =======================================================================================
 * Cubic B-spline coefficients of a volume — csrc/cl_spline.hip
 * =======================================================================================
 * What scipy.ndimage.spline_filter (scipy/ndimage/_interpolation.py, spline_filter1d; src/ni_splines.c: apply_filter with
 * _init_causal_reflect / _init_causal_mirror and their anti-causal counterparts) runs in front of every order-3 interpolation: of
 * map_coordinates as skimage's resize calls it for resample_data_or_seg (3D/d_lka_former/preprocessing/preprocessing.py:130-131), of
 * batchgenerators' interpolate_img in SpatialTransform (data_augmentation_moreDA.py:60-147) and of scipy.ndimage.zoom in test_single_volume
 * (2D/utils.py:63-110).  float64; volumes are ext[3] cells, the last axis contiguous.
 *
 * dlka_spline_pad         padded[in + 2 pad] = x[in] (dtype DLKA_F32 or DLKA_F64) with pad[ax] edge samples on both sides of axis ax; pad 0
 *                         is the cast to float64.
 * dlka_spline_prefilter   in place along one axis of coef[ext]; a line of one cell is left as it is.  boundary: DLKA_SPLINE_REFLECT (scipy's
 *                         'reflect', and its 'nearest' once the array is padded by DLKA_RESAMPLE_SPLINE_PAD edge samples) or
 *                         DLKA_SPLINE_MIRROR ('mirror': what scipy filters with under 'constant', no padding).
 * One launch each, one lane per line, no atomics: results are bitwise reproducible.  Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (an extent
 * < 1, a negative pad, an axis outside 0..2), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (a boundary outside the two, a pad above 64, 2^31 cells or
 * more).  Nothing is launched before the checks pass.  The launches count in dlka_resample_launch_count. */
#define DLKA_RESAMPLE_SPLINE_PAD 12
#define DLKA_SPLINE_REFLECT 0
#define DLKA_SPLINE_MIRROR 1
int dlka_spline_pad(const void *x, double *padded, int dtype, const int64_t *in, const int64_t *pad, void *stream);
int dlka_spline_prefilter(double *coef, const int64_t *ext, int axis, int boundary, void *stream);

/* =======================================================================================
 * Train-time augmentation of a batch of patches — csrc/cl_augment.hip
 * =======================================================================================
 * The apply half of the 3-D trainer's transform chain (get_moreDA_augmentation, 3D/d_lka_former/training/data_augmentation/
 * data_augmentation_moreDA.py:60-147; batchgenerators' SpatialTransform, noise, blur, brightness, contrast, gamma and mirror).  What is
 * random is drawn by the caller on the host; every entry here is a pure function of its inputs.  Volumes are [B][C][D][H][W], W contiguous.
 *
 * storage      dtype is a dlka_dtype or DLKA_AUG_I16 (int16: a float64 result is truncated towards zero, as numpy's astype does).
 * dlka_augment_spatial   per sample b a float64 map maps[12 b ..] (rows of 4: src[d] = m[4d] g0 + m[4d+1] g1 + m[4d+2] g2 + m[4d+3] with
 *              g[e] = index[e] - (out[e] - 1) / 2, formed in the lane: no coordinate grid is stored) and plain[4 b ..] = (flag, lb0, lb1, lb2):
 *              flag != 0 copies the box at lb bit for bit (batchgenerators does not interpolate an unmodified sample).  order 0 / 1 read x;
 *              order 3 reads coef, float64 B-spline coefficients [B*C][src + 2 pad], prepared by dlka_spline_pad and
 *              dlka_spline_prefilter: mode DLKA_AUG_NEAREST with pad 12 and DLKA_SPLINE_REFLECT (scipy's rule), DLKA_AUG_CONSTANT with
 *              pad 0 and DLKA_SPLINE_MIRROR.  The border rule is scipy.ndimage.map_coordinates': 'constant' gives cval wherever a coordinate
 *              is < 0 or > n - 1, 'nearest' clamps the coordinate; taps and weights are scipy's, summed in its order in float64.
 * dlka_augment_spatial_labels   int32 maps.  order 0: the nearest cell (cval outside).  order 1: batchgenerators' per-label rule in one
 *              visit of the 8 neighbours: the largest label whose summed trilinear weight is >= 0.5, else 0; outside under 'constant'
 *              every label's interpolant is cval, which must be < 0.5: 0.
 * dlka_augment_spatial2d, dlka_augment_spatial2d_labels   the same two for the dummy-2D branch of the ACDC trainer (Convert3DTo2DTransform
 *              around SpatialTransform, data_augmentation_moreDA.py:54-75; batchgenerators' augment_spatial with dim == 2): arrays
 *              [B][P][H][W] with d->C = P, the planes of a sample (channels x depth slices), d->src[0..1] = (H, W), d->out[0..1] = (h, w) and
 *              d->src[2] = d->out[2] = 0 (anything else, a 3-D description included: DLKA_ERR_SHAPE).  maps[6 b ..] is the sample's 2 x 3
 *              map (src[d] = (m[3d] g_y + m[3d+1] g_x) + m[3d+2]), plain[3 b ..] = (flag, lb_y, lb_x); every plane of a sample is sampled at
 *              the same in-plane coordinates.  Depth is no interpolation axis: 1 / 4 / 16 taps (outer H, inner W, ((coeff w_y) w_x) summed
 *              left to right, scipy's 2-D map_coordinates), 4 neighbours for order-1 labels, and coef [B*P][H + 2 pad][W + 2 pad] is padded
 *              and filtered along H and W only (the stack of planes as ONE volume through dlka_spline_pad with pad (0, pad, pad) and
 *              dlka_spline_prefilter on axes 1 and 2).  Orders, modes, storage types, border rules and return codes are those above.
 * dlka_augment_gaussian   one axis of scipy.ndimage.gaussian_filter per launch: radius[ch] taps on either side (radius < 0: the channel is
 *              copied) with the weights w[ch][0 .. radius] (centre first, DLKA_AUG_RADIUS_MAX + 1 per channel), mode 'reflect', float64 sums.
 * dlka_augment_channel_stats   stats[4 ch ..] = (sum, sum of squares about the mean, min, max) in float64: lanes, waves, workgroups and the
 *              finish kernel fold in a fixed order, so the result does not depend on scheduling.
 * dlka_augment_pointwise   per channel up to DLKA_AUG_OPS_MAX steps ops[ch][k][6] = (code, p0 .. p4) applied in turn in float64, rounded to
 *              the storage type after each; stats0 / stats1 are dlka_augment_channel_stats results the steps read.  flip[b] bit a: the store
 *              index of spatial axis a is reversed (the mirror).  y must not be x.
 * No atomics anywhere: results are bitwise reproducible.  Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE, DLKA_ERR_DTYPE,
 * DLKA_ERR_UNSUPPORTED (an order, mode or step code outside the lists, 2^31 cells or more per channel, more than 65535 channels, a radius
 * above DLKA_AUG_RADIUS_MAX, cval >= 0.5 for order-1 labels), DLKA_ERR_WORKSPACE.  Nothing is launched before the checks pass. */
#define DLKA_AUG_I16 3
#define DLKA_AUG_CONSTANT 0
#define DLKA_AUG_NEAREST 1
#define DLKA_AUG_RADIUS_MAX 32
#define DLKA_AUG_OPS_MAX 4
enum {
    DLKA_AUG_OP_NONE = 0,
    DLKA_AUG_OP_NOISE = 1,      /* x + noise                                                                        */
    DLKA_AUG_OP_SCALE_ADD = 2,  /* x * p0 + p1                                                                      */
    DLKA_AUG_OP_CONTRAST = 3,   /* clip((x - mean0) * p0 + mean0, min0, max0)                                       */
    DLKA_AUG_OP_GAMMA = 4,      /* s = p1 (+-1): s * (((s x - mn) / (range0 + 1e-7)) ^ p0 * range0 + mn), mn of s x   */
    DLKA_AUG_OP_RETAIN = 5,     /* (x - mean1) / (std1 + 1e-8) * std0 + mean0, population std                       */
    DLKA_AUG_OP_REPLACE = 6     /* x == p0 ? p1 : x                                                                 */
};
typedef struct dlka_augment_desc {
    int32_t B, C, dtype, order, mode, pad;
    int64_t src[3], out[3];
    double cval;
} dlka_augment_desc;
int dlka_augment_spatial(const void *x, const double *coef, void *y, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                         void *stream);
int dlka_augment_spatial_labels(const int32_t *seg, int32_t *out, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                                void *stream);
int dlka_augment_spatial2d(const void *x, const double *coef, void *y, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                           void *stream);
int dlka_augment_spatial2d_labels(const int32_t *seg, int32_t *out, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                                  void *stream);
int dlka_augment_gaussian(const void *x, void *y, int dtype, int64_t channels, const int64_t *ext, int axis, const int32_t *radius,
                          const double *weights, void *stream);
size_t dlka_augment_stats_workspace_bytes(int64_t channels, int64_t cells);
int dlka_augment_channel_stats(const void *x, double *stats, void *workspace, size_t workspace_bytes, int dtype, int64_t channels,
                               int64_t cells, void *stream);
int dlka_augment_pointwise(const void *x, const void *noise, void *y, int dtype, int64_t B, int64_t C, const int64_t *ext, const double *ops,
                           const double *stats0, const double *stats1, const int32_t *flip, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_augment_launch_count(void);

/* =======================================================================================
 * Case preprocessing: nonzero mask with filled holes, crop, intensity normalisation — csrc/cl_preprocess.hip
 * =======================================================================================
 * What the reference runs on one host core per case before a trainer or predict_simple sees it: ImageCropper.crop
 * (3D/d_lka_former/preprocessing/cropping.py:23-150) and the normalisation loop of GenericPreprocessor.resample_and_normalize
 * (preprocessing/preprocessing.py:274-305).  Volumes are [C][d][h][w] float32, w contiguous; label maps int32; a description carries the
 * spatial rank (2 or 3) and ext[3] = (d, h, w), left-padded with 1 for rank 2.
 *
 * dlka_prep_background   cropping.py:26-29 complemented: background[cell] uint8 = 1 where every channel is == 0 (a NaN is != 0, as in numpy).
 *                        The caller labels this map with dlka_cc_components (mask_mode, connectivity 1: scipy's default structure).
 * dlka_prep_fill_bbox    cropping.py:30 (scipy.ndimage.binary_fill_holes) and :35-42 (get_bbox_from_mask) in one pass over the volume:
 *                        a background component is a hole iff none of its cells lies on one of the 2 * rank faces of the array, so
 *                        mask = !background | !(component touches a face).  `labels` is dlka_cc_components' map of the background.
 *                        box[8] int32 (device) = minimum index per axis (3), maximum index per axis (3), number of set cells, unused; an empty
 *                        mask leaves (INT32_MAX x 3, -1 x 3, 0).  Integer atomicMin / atomicMax / atomicAdd only: bitwise reproducible.
 *                        One memset and three launches.  workspace: one byte per cell plus one (dlka_prep_fill_workspace_bytes).
 * dlka_prep_mask_bbox    :35-42 for a given uint8 map (set = value != 0): the same box.  Two launches.
 * dlka_prep_crop         cropping.py:95-115: out[C][box] = data inside [lo, hi) per axis, NaN replaced by 0 when nan_to_zero != 0
 *                        (preprocessing.py:250); seg_out (may be NULL) [max(seg_channels, 1)][box] = with seg_channels > 0 the cropped seg with
 *                        nonzero_label where (seg == 0) & (mask == 0) (:110), otherwise nonzero_label where mask == 0 and 0 elsewhere (:112-115).
 *                        One launch.
 * dlka_prep_channel_stats   completes table[C][DLKA_PREP_REC] float64 (device) = (scheme, lower, upper, mean, sd, use_mask, count, unused): for
 *                        a DLKA_PREP_CT2 channel mean, population sd and count of the cells with (float)lower < x < (float)upper (:292-295), for
 *                        a DLKA_PREP_NONCT channel those of the cells with seg >= 0 (use_mask != 0) or of every cell (:300-304); a DLKA_PREP_CT
 *                        channel keeps the mean and sd it came with.  float64, two passes, folded in a fixed order: bitwise reproducible.
 *                        `seg` is ONE label map (the reference's seg[-1]).  Four launches.  workspace: dlka_prep_stats_workspace_bytes.
 * dlka_prep_normalize    :276-305 for every channel in one launch, each step rounded to float32 and the division IEEE: CT / CT2
 *                        x = min(max(x, (float)lower), (float)upper), (x - (float)mean) / (float)sd, then 0 where use_mask and seg < 0;
 *                        NONCT (x - (float)mean) / ((float)sd + 1e-8f) on the selected cells, 0 elsewhere.  One launch.
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (rank other than 2 or 3, C or an extent < 1, a padded extent != 1, a box outside the array or
 * empty), DLKA_ERR_UNSUPPORTED (C or seg_channels > DLKA_PREP_C_MAX, 2^31 cells or more, out == data for the crop), DLKA_ERR_WORKSPACE.
 * Nothing is launched before the checks pass. */
#define DLKA_PREP_C_MAX 32
#define DLKA_PREP_REC 8
enum { DLKA_PREP_CT = 0, DLKA_PREP_CT2 = 1, DLKA_PREP_NONCT = 2 };
typedef struct dlka_prep_desc {
    int32_t rank, C, seg_channels, nan_to_zero, nonzero_label;
    int64_t ext[3];
    int64_t lo[3], hi[3];                  /* dlka_prep_crop only */
} dlka_prep_desc;
int dlka_prep_background(const float *data, const dlka_prep_desc *d, uint8_t *background, void *stream);
size_t dlka_prep_fill_workspace_bytes(const dlka_prep_desc *d);
int dlka_prep_fill_bbox(const uint8_t *background, const int32_t *labels, const dlka_prep_desc *d, void *workspace, size_t workspace_bytes,
                        uint8_t *mask, int32_t *box, void *stream);
int dlka_prep_mask_bbox(const uint8_t *mask, const dlka_prep_desc *d, int32_t *box, void *stream);
int dlka_prep_crop(const float *data, const int32_t *seg, const uint8_t *mask, const dlka_prep_desc *d, float *out, int32_t *seg_out,
                   void *stream);
size_t dlka_prep_stats_workspace_bytes(const dlka_prep_desc *d);
int dlka_prep_channel_stats(const float *data, const int32_t *seg, const dlka_prep_desc *d, double *table, void *workspace,
                            size_t workspace_bytes, void *stream);
int dlka_prep_normalize(const float *data, const int32_t *seg, const dlka_prep_desc *d, const double *table, float *out, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_prep_launch_count(void);

/* =======================================================================================
 * The 2-D evaluator's slice resampling: scipy.ndimage.zoom of a stack of slices, argmax fused with the zoom back — csrc/cl_zoom2d.hip
 * =======================================================================================
 * test_single_volume (2D/utils.py:63-110) zooms every slice to the patch size at order 3, normalises it, runs the network and zooms the argmax
 * of the logits back at order 0; the train-side __getitem__ (2D/datasets/dataset_synapse.py:109-112) zooms image and label the same way.
 * scipy.ndimage.zoom with its defaults: output index k of an axis n -> m reads the coordinate k * ((n - 1) / (m - 1)); mode 'constant' gives
 * cval = 0 wherever a coordinate is < 0 or > n - 1, at every order.  The caller forms the coordinates in float64 on the host and passes them
 * as tables, rows (out[0] entries) first, then columns (out[1]); stacks are [N][h][w], w contiguous.
 *
 * dlka_zoom2d_spline    taps 4: src = float64 B-spline coefficients [N][in] (dlka_spline_prefilter, DLKA_SPLINE_MIRROR, along axes 1 and 2 of the
 *                       stack); taps 2: src = the raw values in in_dtype (order 1).  start[row] = the first tap (floor(coordinate) - 1, or
 *                       floor(coordinate) for 2 taps) or DLKA_ZOOM2D_OUTSIDE; w4[4 * row + k] = the weights (2 taps: k < 2).  Taps beyond the
 *                       slice are mirrored in the kernel.  The float64 sum t += (c * w_row) * w_col, rows outermost, is rounded once to float32;
 *                       with normalize != 0 the float32 (v - mean) / std follows (one IEEE subtraction, one IEEE division); DLKA_BF16 then
 *                       rounds once more.  DLKA_ZOOM2D_I16 rounds the float64 sum half away from zero and saturates (scipy's rule).
 *                       (in_dtype, out_dtype): taps 4 (DLKA_F64, F32 | BF16 | I16); taps 2 (F32, F32 | BF16), (BF16, BF16), (I16, I16).
 * dlka_zoom2d_nearest   order 0 for elements of elem_bytes (1, 2, 4, 8): y[n][i][j] = x[n][idx[i]][idx[out[0] + j]], 0 where either index is
 *                       outside [0, extent) (the caller writes -1 for a coordinate outside the slice).
 * dlka_zoom2d_argmax    logits [N][K][in] (in_dtype DLKA_F32 or DLKA_BF16, finite), labels [N][out] uint8 = the first maximum over the K planes at
 *                       the source pixel (idx[i], idx[out[0] + j]), 0 where either index is outside.  The [N][in] label map is never written.
 * One launch each, no atomics: results are bitwise reproducible.  Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (N, K or an extent < 1),
 * DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (taps other than 2 or 4, 2^31 cells or more, K > DLKA_ZOOM2D_K_MAX, normalize with I16 or std == 0,
 * output == input).  Nothing is launched before the checks pass. */
#define DLKA_ZOOM2D_I16 3
#define DLKA_ZOOM2D_K_MAX 255
#define DLKA_ZOOM2D_OUTSIDE (-2147483647 - 1)
typedef struct dlka_zoom2d_desc {
    int32_t in_dtype, out_dtype, taps, normalize;
    int64_t N, in[2], out[2];
    float mean, std;
} dlka_zoom2d_desc;
int dlka_zoom2d_spline(const void *src, void *y, const dlka_zoom2d_desc *d, const int32_t *start, const double *w4, void *stream);
int dlka_zoom2d_nearest(const void *x, void *y, const dlka_zoom2d_desc *d, int elem_bytes, const int32_t *idx, void *stream);
int dlka_zoom2d_argmax(const void *logits, uint8_t *labels, const dlka_zoom2d_desc *d, int K, const int32_t *idx, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_zoom2d_launch_count(void);

/* =======================================================================================
 * The trainers' optimizer step: gradient clipping + SGD / Adam / AdamW, learning rate in device memory — csrc/cl_optim.hip
 * =======================================================================================
 * Every reference trainer ends its iteration with SGD: the 3-D trainer with momentum 0.99, Nesterov, weight decay 3e-5
 * (3D/d_lka_former/training/network_training/d_lka_former_trainer_synapse.py:197-205) after clip_grad_norm_(parameters, 12) (:291-309), its
 * learning rate set per epoch by poly_lr (:451); the 2-D trainer with momentum 0.9, weight decay 1e-4 (2D/trainer_MaxViT_deform_LKA.py:114)
 * and a new learning rate every iteration (:145-147); the pancreas trainer likewise (3D/train_pancreas.py:127, :172-175).
 *
 * Multi-tensor entries: host arrays of n per-tensor device pointers and int64 element counts, float32 (DLKA_F32) throughout.  The arrays
 * are read before the entry returns; they are cut into launches of up to DLKA_OPTIM_TENSORS_PER_LAUNCH tensors whose addresses travel in
 * the kernel arguments (a stream capture therefore records them in the kernel nodes: no copy or memset node is added).  A workgroup owns
 * one chunk of DLKA_OPTIM_CHUNK elements of one tensor; the map depends on the counts only.  16-byte accesses where every pointer of a
 * tensor is 16-byte aligned, scalar accesses of the same elements by the same lanes otherwise: both give the same bits.  A tensor is n
 * consecutive elements in memory; zero-element tensors are skipped (their pointers may be NULL).
 *
 * dlka_optim_grad_norm  norm_out[0] (device) = (float)sqrt(sum of squares over all tensors): squares and sums in float64, one partial per
 *                       chunk in `workspace` (dlka_optim_workspace_bytes, 8-byte aligned), added in a fixed order by a finishing launch.  No
 *                       atomics, no host read: bitwise reproducible.  What clip_grad_norm_ returns.
 * dlka_optim_scale      g *= min(1, max_norm / (norm_dev[0] + 1e-6)), the coefficient in float32 as torch forms it; the multiplication always
 *                       happens, so a non-finite norm propagates (torch's error_if_nonfinite=False).  The second half of clip_grad_norm_.
 * dlka_optim_sgd_step   per element, in torch.optim.SGD's order:  g_c = clip ? g * coef : g;  d = g_c + weight_decay * p (weight_decay != 0);
 *                       has_momentum: buf = momentum * buf + d,  u = nesterov ? d + momentum * buf : buf;  else u = d (bufs may be NULL);
 *                       p -= lr_dev[lr_index] * u.  coef as in dlka_optim_scale from norm_dev[0], max_norm.  The gradient is NOT written back.
 *                       Buffers start as zeros (dampening 0: momentum * 0 + d is torch's first-step buf = d); no other dampening.
 * Return codes, in this order, nothing launched before the checks pass: DLKA_ERR_NULL (a table, the descriptor, lr_dev, norm_out, bufs with
 * has_momentum, norm_dev with clip), DLKA_ERR_SHAPE (n < 0, a negative count or lr_index), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (a count or
 * the chunk total above 2^31 - 1), DLKA_ERR_NULL (a NULL address of a tensor with elements), DLKA_ERR_WORKSPACE (NULL, too small, not 8-byte
 * aligned).  n == 0 is DLKA_OK without a launch. */
#define DLKA_OPTIM_TENSORS_PER_LAUNCH 120
#define DLKA_OPTIM_CHUNK 4096
typedef struct dlka_optim_desc {
    int32_t n_tensors, dtype, nesterov, has_momentum, clip;
    float momentum, weight_decay, max_norm;
    int32_t lr_index;
} dlka_optim_desc;
/* bytes of `workspace` for dlka_optim_grad_norm of this list (0 for an invalid or empty one) */
size_t dlka_optim_workspace_bytes(const int64_t *counts, int64_t n);
int dlka_optim_grad_norm(const void *const *grads, const int64_t *counts, int64_t n, int dtype, void *workspace, size_t workspace_bytes,
                         float *norm_out, void *stream);
int dlka_optim_scale(void *const *grads, const int64_t *counts, int64_t n, int dtype, const float *norm_dev, float max_norm, void *stream);
int dlka_optim_sgd_step(void *const *params, const void *const *grads, void *const *bufs, const int64_t *counts, const dlka_optim_desc *d,
                        const float *lr_dev, const float *norm_dev, void *stream);
/* Adam and AdamW on the same tables and partition — what the other reference trainers step with: the 2-D plain-LKA trainer with
 * optim.AdamW(lr, weight_decay=1e-4) and a poly rate written after every iteration (2D/trainer_MaxViT_LKA.py:114, :145-147), the 3-D base
 * trainers with Adam(3e-4, weight_decay=3e-5, amsgrad=True) (3D/d_lka_former/training/network_training/Trainer_synapse.py:270-273,
 * Trainer_acdc.py:269-272).
 *
 * dlka_optim_adam_step  two kinds of launch.  (1) The tick, one workgroup per DLKA_OPTIM_ADAM_TICK_PER_LAUNCH tensors: steps[i][0] += 1 (one
 *                       float32 count per tensor in device memory, torch's `capturable` convention, exact to 2^24 steps) and, with the new
 *                       t, workspace[2 i] = 1 - beta1^t, workspace[2 i + 1] = sqrt(1 - beta2^t), formed in float64 and stored as float32.
 *                       (2) The update, up to DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH tensors a launch, per element in torch.optim.Adam's order:
 *                         g_c = clip ? g * coef : g                                 (coef as in dlka_optim_scale from norm_dev[0], max_norm)
 *                         decoupled (AdamW): p = p * (1 - lr * weight_decay);  else (weight_decay != 0): g_c = g_c + weight_decay * p
 *                         m = m + (g_c - m) * (1 - beta1);   v = beta2 * v + (1 - beta2) * (g_c * g_c)
 *                         amsgrad: vmax = max(vmax, v) (a NaN stays), w = vmax;  else w = v (max_exp_avg_sq may be NULL)
 *                         p = p - ((lr / workspace[2 i]) * m) / (sqrt(w) / workspace[2 i + 1] + eps),   lr = lr_dev[lr_index]
 *                       every product, quotient and sum rounded to float32 on its own; 1 - beta1 and 1 - beta2 are formed in float64.  No
 *                       workgroup of the update writes a count or reads the host; the gradient is NOT written back.  A captured call
 *                       advances the counts at every replay.  exp_avg, exp_avg_sq, max_exp_avg_sq start as zeros, the counts as 0.
 *                       `workspace`: dlka_optim_adam_workspace_bytes(n_tensors) bytes, 4-byte aligned, the caller's until the stream has
 *                       run the call.  Every listed tensor needs a count address, a zero-element one too (torch counts its steps).
 * Return codes as above: DLKA_ERR_NULL (a table, the descriptor, lr_dev, norm_dev with clip, max_exp_avg_sq with amsgrad), DLKA_ERR_SHAPE
 * (n_tensors < 0, a negative count or lr_index, a beta outside [0, 1), eps or weight_decay below 0), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED,
 * DLKA_ERR_NULL (a NULL address of a tensor with elements, a NULL count address), DLKA_ERR_WORKSPACE.  n_tensors == 0: DLKA_OK, no launch. */
#define DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH 80
#define DLKA_OPTIM_ADAM_TICK_PER_LAUNCH 448
typedef struct dlka_optim_adam_desc {
    int32_t n_tensors, dtype, decoupled, amsgrad, clip;
    double beta1, beta2, eps, weight_decay;   /* torch holds them as doubles; 1 - beta is formed before the rounding to float32 */
    float max_norm;
    int32_t lr_index;
} dlka_optim_adam_desc;
size_t dlka_optim_adam_workspace_bytes(int64_t n_tensors);
int dlka_optim_adam_step(void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq, void *const *max_exp_avg_sq,
                         void *const *steps, const int64_t *counts, const dlka_optim_adam_desc *d, const float *lr_dev, const float *norm_dev,
                         void *workspace, size_t workspace_bytes, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_optim_launch_count(void);

/* =======================================================================================
 * The 3-D trainer's batch loader: oversampled patch batches and class locations — csrc/cl_dataload.hip
 * =======================================================================================
 * DataLoader3D.generate_train_batch (3D/d_lka_former/training/dataloading/dataset_loading.py:223-379) cuts one box per sample out of a
 * case [C + 1][x][y][z] float32 (the label map is the last channel) and pads what falls outside; GenericPreprocessor._run_internal
 * (preprocessing/preprocessing.py:333-348) records, per class, the cells the loader's foreground oversampling centres a box on.
 *
 * dlka_load_crop_batch     data [B][C][patch] and seg [B][1][patch] of B <= DLKA_LOAD_B_MAX samples in ONE launch.  Sample b reads the case
 *                          at sample[b].data with extents sample[b].ext; output cell p takes case cell p + sample[b].lb.  Outside the case
 *                          the data takes `constant` (DLKA_LOAD_CONSTANT) or the nearest cell of the case (DLKA_LOAD_EDGE: np.pad's 'edge');
 *                          the label map always takes -1.  The description is a HOST structure; the library hands it to the kernel by
 *                          value, so a call copies nothing to the device.  Cells are moved as bits.  A larger batch is the caller's to cut.
 * dlka_load_class_counts   one read of a label map [x][y][z] (DLKA_LOAD_F32 with integer values, or DLKA_LOAD_I32) for all K <=
 *                          DLKA_LOAD_K_MAX distinct class_id: totals[K] int32 (device) = cells per class, and in `workspace`
 *                          (dlka_load_counts_workspace_bytes, kept for the selection) the exclusive offset of every tile per class.  Cells
 *                          with any other label are ignored.  Two launches.
 * dlka_load_class_select   out[count][3] int32 (device) = the (x, y, z) of cell number sel_rank[j], in raster order (numpy.argwhere's), among
 *                          the cells of class_id[sel_slot[j]].  `offsets` is the workspace dlka_load_class_counts filled for the same map
 *                          and description, `totals` its totals read back (host, int64); `workspace`: dlka_load_select_workspace_bytes.
 *                          The order comes from the scan of the tile counts; there is no atomic: bitwise reproducible.  A slot or rank
 *                          that does not exist gives (-1, -1, -1).  Two launches.
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (B, C, K, count or an extent < 1, a class_id listed twice, totals no map of these extents
 * has), DLKA_ERR_DTYPE, DLKA_ERR_UNSUPPORTED (B > DLKA_LOAD_B_MAX, K > DLKA_LOAD_K_MAX, another mode, a case or label map of 2^31 cells per
 * channel or more, a patch extent or |lb| above 2^30, |class_id| above 2^24), DLKA_ERR_WORKSPACE.  Nothing is launched before the checks pass. */
#define DLKA_LOAD_B_MAX 32
#define DLKA_LOAD_K_MAX 32
enum { DLKA_LOAD_CONSTANT = 0, DLKA_LOAD_EDGE = 1 };
enum { DLKA_LOAD_F32 = 0, DLKA_LOAD_I32 = 1 };
typedef struct dlka_load_sample {
    const float *data;
    int64_t ext[3], lb[3];
} dlka_load_sample;
typedef struct dlka_load_crop_desc {
    int32_t B, C, mode;
    float constant;
    int64_t patch[3];
    dlka_load_sample sample[DLKA_LOAD_B_MAX];
} dlka_load_crop_desc;
typedef struct dlka_load_classes_desc {
    int32_t K, dtype;
    int64_t ext[3];
    int64_t class_id[DLKA_LOAD_K_MAX];
} dlka_load_classes_desc;
int dlka_load_crop_batch(const dlka_load_crop_desc *d, float *data, float *seg, void *stream);
size_t dlka_load_counts_workspace_bytes(const dlka_load_classes_desc *d);
int dlka_load_class_counts(const void *seg, const dlka_load_classes_desc *d, void *workspace, size_t workspace_bytes, int32_t *totals,
                           void *stream);
size_t dlka_load_select_workspace_bytes(const dlka_load_classes_desc *d, const int64_t *totals);
int dlka_load_class_select(const void *seg, const dlka_load_classes_desc *d, const void *offsets, size_t offsets_bytes, const int64_t *totals,
                           void *workspace, size_t workspace_bytes, const int32_t *sel_slot, const int32_t *sel_rank, int64_t count,
                           int32_t *out, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_load_launch_count(void);

/* =======================================================================================
 * The dataset fingerprint: DatasetAnalyzer's intensity statistics and unique labels — csrc/cl_dataset_stats.hip
 * =======================================================================================
 * DatasetAnalyzer (3D/d_lka_former/experiment_planning/DatasetAnalyzer.py) samples every tenth foreground voxel of every case
 * (_get_voxels_in_foreground, :161-166), takes median, mean, sd, min, max and the 99.5 / 0.5 percentiles of the samples of a case and of
 * the whole dataset (_compute_stats, :168-179; collect_intensity_properties, :181-223), and lists the labels of a case (_get_unique_labels,
 * :76-79).  All device arrays below are contiguous; a label map is float32 with integer values (DLKA_DSTATS_F32, the last channel of a
 * cropped case) or int32 (DLKA_DSTATS_I32) and is read in that type.
 *
 * dlka_dstats_fg_count       :164: *count (device, int64) = cells of the label map [ext] with label > 0, and in `workspace`
 *                            (dlka_dstats_fg_workspace_bytes, kept for the sample) the exclusive offset of every tile.  Two launches.
 * dlka_dstats_fg_sample      :163-165: out[c * out_stride + out_offset + j] = data[c][mask][::step][j] for the C <= DLKA_PREP_C_MAX volumes
 *                            data [C][ext] and j < out_count, in raster order, fixed by the scan: no atomic.  `offsets` is the workspace
 *                            dlka_dstats_fg_count filled for the same map and description; out_count = ceil(count / step) as the host read
 *                            it (a smaller value writes fewer, a larger one no more than exist).  Writing at out_offset is what lets the
 *                            samples of a dataset's cases land in one buffer, case after case.  One launch.
 * dlka_dstats_moments        :173-174: result[4] (device, float64) = n, np.mean, np.std (ddof 0), the number of NaNs of x[n], accumulated in
 *                            float64 in a fixed order, two passes (mean, then centred squares).  Four launches.
 * dlka_dstats_select         :172,175-178: values[j] (device) = the ranks[j]-th smallest (0-based) of x[n], NaNs sorting last as numpy sorts
 *                            them (a rank among them gives a NaN) and -0.0 counting as +0.0, which is what a zero comes back as;
 *                            *nan_count (device, int64, may be NULL) = the NaNs of x.  `ranks` is a HOST array of n_ranks <=
 *                            DLKA_DSTATS_RANKS_MAX ranks.  A radix select, 4 passes of 8 bits over x, which is only read; `workspace`:
 *                            dlka_dstats_select_workspace_bytes.  Nine launches, whatever n and the ranks are.
 * dlka_dstats_unique_labels  :78: bitmap[DLKA_DSTATS_LABEL_WORDS] (device): bit (v - DLKA_DSTATS_LABEL_MIN) % 32 of word
 *                            (v - DLKA_DSTATS_LABEL_MIN) / 32 is set for every label v of the map; the LAST word is nonzero when a label lies
 *                            outside DLKA_DSTATS_LABEL_MIN .. DLKA_DSTATS_LABEL_MAX or is no integer.  One launch.
 * Integer atomics only: every result is bitwise reproducible.
 * Return codes: DLKA_ERR_NULL, DLKA_ERR_SHAPE (rank outside 2..3, rank 2 with ext[0] != 1, C, step, n, n_ranks, out_count or an extent < 1,
 * a rank outside 0 .. n - 1, out_count beyond ceil(cells / step), out_offset < 0 or out_offset + out_count > out_stride), DLKA_ERR_DTYPE,
 * DLKA_ERR_UNSUPPORTED (C > DLKA_PREP_C_MAX, n_ranks > DLKA_DSTATS_RANKS_MAX, a map of 2^31 cells or more, step above 2^31 - 1, n of 2^32
 * or more), DLKA_ERR_WORKSPACE.  Nothing is launched before the checks pass. */
#define DLKA_DSTATS_RANKS_MAX 8
#define DLKA_DSTATS_LABEL_MIN (-1)
#define DLKA_DSTATS_LABEL_MAX 255
#define DLKA_DSTATS_LABEL_WORDS 10
enum { DLKA_DSTATS_F32 = 0, DLKA_DSTATS_I32 = 1 };
typedef struct dlka_dstats_desc {
    int32_t rank, C, label_dtype, reserved;   /* rank 2: ext[0] = 1; C: volumes of the sample (1 where none is read) */
    int64_t ext[3];
    int64_t step;                             /* every step-th foreground cell (1 where none is sampled) */
} dlka_dstats_desc;
size_t dlka_dstats_fg_workspace_bytes(const dlka_dstats_desc *d);
int dlka_dstats_fg_count(const void *seg, const dlka_dstats_desc *d, void *workspace, size_t workspace_bytes, int64_t *count, void *stream);
int dlka_dstats_fg_sample(const float *data, const void *seg, const dlka_dstats_desc *d, const void *offsets, size_t offsets_bytes,
                          int64_t out_count, float *out, int64_t out_stride, int64_t out_offset, void *stream);
size_t dlka_dstats_moments_workspace_bytes(int64_t n);
int dlka_dstats_moments(const float *x, int64_t n, void *workspace, size_t workspace_bytes, double *result, void *stream);
size_t dlka_dstats_select_workspace_bytes(void);
int dlka_dstats_select(const float *x, int64_t n, const int64_t *ranks, int32_t n_ranks, void *workspace, size_t workspace_bytes,
                       float *values, int64_t *nan_count, void *stream);
int dlka_dstats_unique_labels(const void *seg, const dlka_dstats_desc *d, uint32_t *bitmap, void *stream);
/* Diagnostics: kernel launches so far (this process) of the entries above. */
long dlka_dstats_launch_count(void);

/* =======================================================================================
 * Efficient paired attention (UNETR++ EPA, the reference's TransformerBlock: synapse/transformerblock.py:68-138) — csrc/cl_epa.hip
 * =======================================================================================
 * float32; D = C / heads in {8, 16, 32, 64}, P in {32, 64}, any N.  Per sample b and head h, with Q, K, Vc, Vs the four D-wide column
 * groups of qkvv [B][N][4][heads][D] (the Linear's own output, read in place):
 *   rq_i = 1 / max(|Q[:, i]|, 1e-12) over the N tokens, rk_j likewise;   Qh = Q rq, Kh = K rk
 *   A = softmax_j((Qh^T Kh)[i][j] temperature[h]);   x_ca[b][n][h D + i] = sum_j (A m1)[i][j] Vc[n][j]
 *   S[n] = softmax_p(Qh[n] . kp[b][h D + :][p] temperature2[h]);   Y[n][i] = sum_p (S m2)[n][p] vp[b][h D + i][p], stored to
 *   x_sa at flat offset ((b D + i) heads + h) N + n — what the reference's permute(0, 3, 1, 2).reshape(B, N, C) of [B][heads][N][D] holds.
 * kp, vp [B][C][P]: the projections of K and Vs over the tokens (a GEMM the caller runs).  temperature, temperature2 [heads].
 * m1: optional float multipliers [B][heads][D][D]; m2: optional keep bytes [B][heads][N][P], a set byte multiplies by m2_scale.
 * saved: the forward call's statistics (saved_bytes), handed to the backward call unchanged.  Backward: g_x_sa in x_sa's layout, g_x_ca [B][N][C];
 * g_qkvv [B][N][4 C] is fully overwritten with the gradient through Q, the channel branch's K and Vc (slot 3, Vs, is zero: Vs and the spatial
 * branch's K are reached through vp / kp, whose gradients g_vp / g_kp [B][C][P] the caller carries through its GEMMs); g_temperature_bh and
 * g_temperature2_bh [B][heads] are per sample and are summed over B by the caller.  Sums over tokens are per-workgroup partial tiles folded in
 * workgroup order, no float atomics: identical calls give identical bits.  Return codes: DLKA_ERR_NULL, DLKA_ERR_DTYPE, DLKA_ERR_SHAPE (a size
 * < 1), DLKA_ERR_UNSUPPORTED (a width outside the set, 2^31 elements or more in qkvv or in the N x P map), DLKA_ERR_WORKSPACE. */
int dlka_epa_supported(int C, int heads, int P, int dtype);
size_t dlka_epa_saved_bytes(int B, int C, int heads);
size_t dlka_epa_workspace_bytes(int B, int N, int C, int heads, int P, int backward);
int dlka_epa_attention_forward(const void *qkvv, const void *kp, const void *vp, const void *temperature, const void *temperature2, const void *m1,
                               const void *m2, float m2_scale, void *x_sa, void *x_ca, void *saved, void *workspace, size_t workspace_bytes, int B, int N,
                               int C, int heads, int P, int dtype, void *stream);
int dlka_epa_attention_backward(const void *qkvv, const void *kp, const void *vp, const void *temperature, const void *temperature2, const void *m1,
                                const void *m2, float m2_scale, const void *saved, const void *g_x_sa, const void *g_x_ca, void *g_qkvv, void *g_kp,
                                void *g_vp, void *g_temperature_bh, void *g_temperature2_bh, void *workspace, size_t workspace_bytes, int B, int N, int C,
                                int heads, int P, int dtype, void *stream);

/* =======================================================================================
 * Launch trace — measurement aid (no reference counterpart; the reference has no profiling hooks)
 * =======================================================================================
 * Between dlka_trace_start and dlka_trace_stop every kernel launch of the library is followed by a HIP timing event on the
 * launch's own stream; record i = (kernel name, milliseconds since the previous record).  bench.py runs the timed step once
 * more under the trace to report the roofline of the kernels the step REALLY launches.  dlka_trace_mark inserts a record
 * without a kernel (name "(mark)") to separate phases.  Not thread-safe; illegal during hipGraph capture.  */
int dlka_trace_start(int max_events, void *stream);
int dlka_trace_mark(void *stream);
int dlka_trace_stop(void);                 /* synchronises with the last record; DLKA_ERR_WORKSPACE if records were dropped */
int dlka_trace_count(void);
int dlka_trace_get(int i, char *name, size_t name_cap, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* DLKA_H_ */
