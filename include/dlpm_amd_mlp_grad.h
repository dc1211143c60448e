/* dlpm_amd_mlp_grad.h -- gradients of the 2-D toy net (MLPModel) at any architecture in libdlpm_amd: same library, same ABI version
 * as dlpm_amd.h, which this header includes; the functions live here so that the tables of dlpm_amd_train.h and dlpm_amd_mlp.h stay
 * as they are.
 *
 * The five entry points take ANY dlpm_mlp handle.  For a handle on the lane kernels (the shipped 64-unit architecture) each one
 * forwards to its counterpart of dlpm_amd_train.h -- dlpm_mlp_param_floats, dlpm_mlp_export_params_f32,
 * dlpm_mlp_import_params_f32, dlpm_mlp_backward_workspace_bytes, dlpm_mlp_backward_f32 -- with the same bits and error codes.
 * For a handle on the general forward (dlpm_amd_mlp.h) they run the backward of that forward on the fp32 MFMA.  The fused trainer
 * of dlpm_amd_train.h keeps refusing such a handle; this header is what an autograd bridge calls.
 *
 * Supported range of the general backward: the whole range of the general forward,
 *     1 <= nfeatures <= 64,  1 <= nunits <= 1024,  1 <= time_emb_size <= 1024,  nblocks >= 0,  LayerNorm and skip on or off.
 * A workgroup of the backward takes the LDS of the forward at the same tile height (its dY tile lies in the forward's activation
 * image, dL/d(time embedding) in the time-embedding image), so every net dlpm_mlp_create_ex accepts has a backward; a tile that
 * does not fit 160 KB is DLPM_ERR_UNSUPPORTED with the byte count, from the workspace query and the backward, before any launch.
 *
 * The flat parameter vector is torch.nn.utils.parameters_to_vector(model.parameters()) of that architecture: named_parameters()
 * order (group_norm_in, time_emb, time_mlp.2, linear_in, then per block group_norm1, group_norm2, mlp_1.1, t_proj.1, mlp_2.1 for
 * midblocks.0 .. and outblocks_mean.0, then outblocks_mean.1), weight before bias, torch's [out][in] layout, every alias once; a
 * net without LayerNorm has no group_norm tensors in it.
 *
 * No entry point synchronises, reads a device value on the host or uses a floating-point atomic; every sum is taken in a fixed
 * order, so the same inputs give the same bits on every call and at every tile height. */
#ifndef DLPM_AMD_MLP_GRAD_H
#define DLPM_AMD_MLP_GRAD_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The length P of the flat vector (55 010 for the shipped net); < 0 for a null handle.  Needs no dlpm_mlp_finalize. */
int64_t dlpm_mlp_grad_param_floats(const dlpm_mlp *m);

/* flat_dev[P] <- the net's parameters, gathered on the device.  DLPM_ERR_ARG for a null pointer or n != P, DLPM_ERR_STATE before
 * dlpm_mlp_finalize. */
int dlpm_mlp_grad_export_params_f32(dlpm_mlp *m, float *flat_dev, int64_t n, dlpm_stream_t stream);

/* The net's parameters <- flat_dev[P], on the stream, without the host: one index per real parameter scatters it into the
 * forward's operand blob, into the transposed operands the backward multiplies by, and into the padded vectors; padded elements
 * stay exactly 0.  The tensors dlpm_mlp_set_param was given are not updated: a later dlpm_mlp_finalize uploads those.  A
 * sampler created on this handle that has captured a graph must be dropped by the caller.  Refusals as for export. */
int dlpm_mlp_grad_import_params_f32(dlpm_mlp *m, const float *flat_dev, int64_t n, dlpm_stream_t stream);

/* Bytes of workspace dlpm_mlp_grad_backward_f32 needs for `rows` rows; < 0 for a null handle or rows <= 0 (or
 * DLPM_ERR_UNSUPPORTED, also negative, where the tile does not fit the LDS).  General handles: per row 5 records of the padded
 * time_emb_size, 4 + 10 (nblocks + 1) records of the padded nunits and 4 (nblocks + 2) scalars, then at most 16 fp64 copies of
 * the gradient -- see dlpm_mlp_grad_backward_f32. */
int64_t dlpm_mlp_grad_workspace_bytes(const dlpm_mlp *m, int64_t rows);

/* Given dout = dL/d(output) [rows,F] at the inputs x [rows,F], t [rows]: grad_flat[P] = dL/d(parameter) in the flat order above
 * and, when dx_dev is given, dx [rows,F] = dL/dx.
 * General handles, three steps.  (1) The row pass: the forward's tiles (one workgroup per 16 or 32 rows, a wave the same column
 * tiles of every layer) recompute the forward with the very operations of dlpm_mlp_forward, leave per row every Linear's input,
 * every LayerNorm's normalised value and 1 / sigma and every dL/d(pre-activation) in the workspace, and walk back; every hidden
 * dX = dY W is v_mfma_f32_16x16x4_f32 against the transposed operand.  dx of a row depends on that row alone.  Rows past the end of
 * a ragged tile write nothing.  (2) The weight pass: every dW = dY^T A on the same MFMA, the reduction over the rows.  The rows
 * are cut into chunks of 64; a chunk accumulates in fp32, rows in order.  The chunks are dealt in order to at most 16 slots of
 * ceil(chunks / 16) consecutive chunks each; a slot adds its chunk partials in chunk order in fp64.  Biases and LayerNorm weights
 * and biases, single columns, are summed in fp64 throughout.  (3) The slots are added in slot order in fp64 and rounded once.
 * So the workspace holds at most 16 gradient-sized partial buffers whatever the row count.
 * DLPM_ERR_ARG for a null pointer (dx_dev may be null), rows <= 0 or a workspace that is not 8-byte aligned, DLPM_ERR_UNSUPPORTED
 * where the tile does not fit the LDS, DLPM_ERR_NOMEM for a short workspace, DLPM_ERR_STATE before dlpm_mlp_finalize -- all before
 * any launch. */
int dlpm_mlp_grad_backward_f32(dlpm_mlp *m, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                               float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_MLP_GRAD_H */
