/* dlpm_amd_chains.h -- the two-chain sampler step's entry points of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which
 * this header includes): how a batch is laid out as independent half-batch chains, and what a sampler reports about them.
 *
 * dlpm_sampler_steps enqueues one reverse step of the UNet sampler as TWO chains of kernels, rows [0, B/2) on the stream of the step
 * and rows [B/2, B) on a second stream the sampler owns, forked and joined with events -- under capture, two parallel branches of the
 * one graph.  Nothing of a step crosses samples, every chain launches the kernels the whole batch would (kernel choice follows the
 * declared dispatch batch, dlpm_unet_set_conv_policy), so the state has the bits of the one-chain step.  DLPM_SAMPLER_CHAINS=1 keeps
 * every step on one chain. */
#ifndef DLPM_AMD_CHAINS_H
#define DLPM_AMD_CHAINS_H

#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DLPM_MAX_CHAINS 2

/* The workspace of a batch that is walked as `chains` (1..DLPM_MAX_CHAINS, <= B) independent row ranges, each in an arena of its own:
 * chain c covers rows [rows_off[c], rows_off[c] + rows[c]) -- B / chains each, the remainder to the last chains, so B = 5 is 2 + 3 --
 * in the arena [arena_off[c], arena_off[c] + arena_bytes[c]) of one allocation, arena_bytes[c] = dlpm_unet_workspace_bytes(net,
 * rows[c]).  Returns the bytes of the arenas together; *single_bytes = dlpm_unet_workspace_bytes(net, B), and *slack_bytes = the
 * rounding of the arena's 256-byte blocks, by which alone the former may exceed the latter (both optional).  Pure host arithmetic on
 * the launch plan.  -1 on error. */
int64_t dlpm_unet_chain_workspace(const dlpm_unet *net, int64_t B, int32_t chains, int64_t *rows_off, int64_t *rows,
                                  int64_t *arena_off, int64_t *arena_bytes, int64_t *single_bytes, int64_t *slack_bytes);

/* How many chains the next plain step of this sampler (dlpm_sampler_steps) is enqueued as: 2 on the UNet's fused-head path at B >= 2,
 * 1 everywhere else and under DLPM_SAMPLER_CHAINS=1. */
int32_t dlpm_sampler_chains(const dlpm_sampler *s);
/* How many graphs this sampler has captured so far: reseeding, set_state and new labels capture none. */
int64_t dlpm_sampler_graph_captures(const dlpm_sampler *s);

#ifdef __cplusplus
}
#endif
#endif
