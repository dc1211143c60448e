/* dlpm_amd_mlp.h -- the 2-D toy net (MLPModel) at any architecture in libdlpm_amd: same library, same ABI version as dlpm_amd.h,
 * which this header includes; the functions live here so that the table of dlpm_amd.h stays as it is.
 *
 * dlpm/models/Model.py:28-39 takes nunits, nblocks, time_emb_size, group_norm and skip_connection as free parameters.  The library
 * has two forwards for it.  The lane kernels of dlpm_amd.h map 64 hidden units onto the 64 lanes of a wavefront and take the
 * shipped architecture: nunits == 64, time_emb_size <= 64, LayerNorm and skip connections.  The general forward takes everything
 * else in
 *     1 <= nfeatures <= 64,  1 <= nunits <= 1024,  1 <= time_emb_size <= 1024,  nblocks >= 0,  LayerNorm and skip on or off:
 * one workgroup owns a tile of 16 or 32 rows for the whole net, the activations stay in LDS and registers, and every Linear with a
 * hidden dimension is v_mfma_f32_16x16x4_f32 products (exact fp32) against a zero-padded operand blob that dlpm_mlp_finalize packs
 * once.  No floating-point atomic; every sum in a fixed order; a row's bits depend on that row alone -- not on the batch, on its
 * place in the tile or the grid, on the tile height or on what other rows hold.
 *
 * dlpm_mlp_forward routes by handle.  For a handle on the general forward, dlpm_mlp_sample_steps_f32 (the one-launch loop) and
 * the training entry points of dlpm_amd_train.h (dlpm_mlp_param_floats, dlpm_mlp_backward_workspace_bytes, dlpm_mlp_backward_f32,
 * dlpm_mlp_export_params_f32, dlpm_mlp_import_params_f32) return DLPM_ERR_UNSUPPORTED with a message (the gradients of such a
 * net: dlpm_amd_mlp_grad.h); a sampler on such a handle takes the per-step path (forward + update kernel in the captured graph). */
#ifndef DLPM_AMD_MLP_H
#define DLPM_AMD_MLP_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum dlpm_mlp_flags {
    DLPM_MLP_NO_LAYERNORM = 1,  /* group_norm: false -- nn.Identity in place of every LayerNorm; the state_dict then has no
                                   group_norm* keys and no inblock.1.*, mlp_1.2.*, mlp_2.2.* aliases, and dlpm_mlp_set_param
                                   refuses them                                                                               */
    DLPM_MLP_NO_SKIP = 2,       /* skip_connection: false                                                                     */
    DLPM_MLP_FORCE_GENERAL = 4, /* the general forward even for the shipped architecture (for comparison)                     */
    DLPM_MLP_TILE_16 = 8,       /* general forward: 16-row tiles whatever the batch (the results are the same bits)           */
    DLPM_MLP_TILE_32 = 16       /* general forward: 32-row tiles whatever the batch; DLPM_ERR_UNSUPPORTED where they do not
                                   fit the LDS.  Without either flag a call takes 32-row tiles where they fit and fill the
                                   chip (at least 256 of them), 16-row tiles otherwise: a row's bits do not depend on it      */
};

/* dlpm_mlp_create with the architecture switches; dlpm_mlp_create(...) is dlpm_mlp_create_ex(..., 0, out).
 * DLPM_ERR_ARG for a null `out`, nfeatures < 1, nunits < 1, time_emb_size < 1, nblocks < 0, an unknown flag or both tile flags;
 * DLPM_ERR_UNSUPPORTED beyond the ranges above, or when a workgroup's tile does not fit 160 KB of LDS. */
int dlpm_mlp_create_ex(int32_t nfeatures, int32_t nunits, int32_t nblocks, int32_t time_emb_size, int32_t flags, dlpm_mlp **out);

/* Rows of the tallest tile one workgroup may own in the general forward (32, or 16 where 32 do not fit the LDS or
 * DLPM_MLP_TILE_16 is set); 0 for a handle on the lane kernels; < 0 for a null handle.  Needs no dlpm_mlp_finalize. */
int32_t dlpm_mlp_tile_rows(const dlpm_mlp *net);

/* Bytes of LDS of one workgroup of the general forward at that tile; 0 for a handle on the lane kernels; < 0 for a null handle. */
int64_t dlpm_mlp_lds_bytes(const dlpm_mlp *net);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_MLP_H */
