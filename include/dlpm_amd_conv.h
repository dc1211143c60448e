/* dlpm_amd_conv.h -- a 3x3 stride-1 convolution launch under a DECLARED policy, at the kernel level (same library, same ABI version as
 * dlpm_amd.h, which this header includes; the two functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * dlpm_conv2d_f32 never declares a dispatch batch, so it cannot reach the launches that exist only under one: the split-K grid copies
 * of the F(2x2) kernel and of the narrow F(4x4) shapes (ConvRoute::ksplit = 2, 4, 8, conv_splitk.hip) and the 64- / 32-channel n-tiles
 * of a Cout % 128 == 0 layer.  These two entry points carry the policy of dlpm_unet_set_conv_policy -- a generation and a dispatch
 * batch -- down to ONE launch: the layer gets the weight layouts the UNet would build for it under that declaration (conv.h:
 * conv_layouts and its table, which dlpm_unet_finalize and dlpm_unet_set_conv_policy ask too), conv_route decides, and the launch runs through the function the
 * plan runs (conv_splitk.hip: launch_conv_splitk).  Test / bring-up entry points, like dlpm_conv2d_f32.
 *
 * Both take launches with ksize = 3, stride = 1, NHWC on both sides, Cout > 4, force_direct = 0 (upsampling included); anything else
 * is DLPM_ERR_UNSUPPORTED.  generation is a dlpm_conv_generation, dispatch_batch >= 0 (0: none declared). */
#ifndef DLPM_AMD_CONV_H
#define DLPM_AMD_CONV_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the kernel family of a route, in the order of the selector cascade (conv.h: ConvFamily) */
typedef enum dlpm_conv_family {
    DLPM_CONV_FAMILY_HEAD_FUSED = 0, DLPM_CONV_FAMILY_HEAD_GEMM = 1, DLPM_CONV_FAMILY_HEAD = 2, DLPM_CONV_FAMILY_SPLIT = 3,
    DLPM_CONV_FAMILY_WINO4SP = 4, DLPM_CONV_FAMILY_WINO4 = 5, DLPM_CONV_FAMILY_WINO = 6, DLPM_CONV_FAMILY_IGEMM = 7,
    DLPM_CONV_FAMILY_STEM = 8, DLPM_CONV_FAMILY_DIRECT = 9
} dlpm_conv_family;

typedef struct dlpm_conv_route {
    int32_t family;          /* dlpm_conv_family                                                                              */
    int32_t bh, bw, nimg;    /* Winograd families: tiles per block (rows, columns), images per block                          */
    int32_t nq;              /* Winograd families: n-tile width in channels                                                   */
    int32_t stats_px;        /* pixels behind one statistics partial; 0: this launch emits none (every split-K launch)        */
    int32_t ksplit;          /* split-K factor S (1: none)                                                                    */
    int32_t reserved;
    int64_t grid;            /* Winograd families under a declared batch: workgroups at dispatch_batch                        */
    int64_t scratch_floats;  /* what dlpm_conv_policy_f32 needs as scratch_dev for this layer under this declaration          */
    int64_t partial_floats;  /* ... and as partial_dev: S * B * Hout * Wout * Cout where S > 1, else 0                        */
} dlpm_conv_route;

/* The route of the launch, and the buffer sizes dlpm_conv_policy_f32 asks for.  Host arithmetic only: no pointer of args is followed,
 * no GPU is touched (the data pointers may be null).  DLPM_ERR_ARG for a null argument, an unknown generation, a negative
 * dispatch_batch, non-positive sizes or an output size that is not the input's (twice it when upsample is set). */
int dlpm_conv_policy_route(const dlpm_conv_args *args, int32_t generation, int64_t dispatch_batch, dlpm_conv_route *route);

/* The launch.  scratch_dev (args->scratch_floats floats, at least route.scratch_floats) receives the weight layouts, built from the
 * OIHW weight on `stream` as dlpm_conv2d_f32 does.  A split-K route (S = route.ksplit > 1) writes its S partial outputs, NHWC
 * [S][B][Hout][Wout][Cout] with copy s covering input channels [s Cin / S, (s + 1) Cin / S) and neither bias nor residual, into
 * partial_dev (partial_floats floats, at least route.partial_floats; it still holds them after the call) and forms
 *     out = (((part[0] + part[1]) + part[2]) + ...) + bias + residual
 * in that order; without a split partial_dev is not touched and may be null.  stats_out / stats_px (both or neither) as in
 * dlpm_conv2d_stats_f32.  *route (optional) receives the route the launch took.
 * Before anything is enqueued: DLPM_ERR_NOMEM for a scratch or partial buffer that is too small; DLPM_ERR_UNSUPPORTED when statistics
 * are asked of a route with stats_px == 0 (nothing is written); DLPM_ERR_ARG as above and for a null src0 / weight / out / scratch_dev. */
int dlpm_conv_policy_f32(const dlpm_conv_args *args, int32_t generation, int64_t dispatch_batch, float *scratch_dev, float *partial_dev,
                         int64_t partial_floats, float *stats_out, int32_t *stats_px, dlpm_conv_route *route, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_CONV_H */
