/*
 * locostate.h — C-ABI of a batch's STATE ON DEVICE BUFFERS, served by "liblocohip.so" beside include/locohip.h: read, set and restart
 * environments without leaving the device or the caller's stream (lm_set_state, lm_get_state, lm_set_goal and lm_set_activation of
 * locohip.h take host pointers and wait for the device). A header and a prefix of its own, like locotape.h and locovec.h: the list of
 * lm_ names that locohip.h declares stays exactly what it is. One kernel launch each (csrc/lm_state_io.h).
 *
 *   ls_get_state_device   <- reading data.qpos / data.qvel / data.act of every environment, as device tensors
 *   ls_set_state_device   <- LocoEnv.reset's state write (the reference's base.py:178-203), from rows the caller holds on the device
 *   ls_restart_device     <- the per-environment reset from a trajectory sample (trajectory.py:236-273 + base.py:478-497), on request
 *
 * Every pointer is a DEVICE pointer on the batch's device, taken as given like those of lm_step_device; rows are row-major. Functions
 * return 0 on success, non-zero on error; lm_last_error() returns the message for the calling thread.
 */
#ifndef LOCOSTATE_H
#define LOCOSTATE_H

#include <stdint.h>
#include "locohip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_mask: [n_envs] bytes, non-zero = this environment; NULL = all. The mask alone decides which environments are written, whether or
   not an active list is set (lm_batch_set_active).
     ls_get_state_device  qpos / qvel [n_envs][nv], muscle activations [n_envs][na], goal [n_envs][ngoal], the episode's step
                          [n_envs] int32 and the episode count [n_envs] uint32 -> the caller's buffers; each may be NULL, not all.
     ls_set_state_device  for every masked environment what lm_set_state does, from device rows d_qpos / d_qvel [n_envs][nv] (both
                          needed; rows of unmasked environments are not read): positions and velocities written; solver warm start,
                          self-collision slack, the episode's step and the replay prediction mark cleared; muscle activations zeroed
                          (mj_resetData, the reference's base.py:178-203) — or, with d_act [n_envs][na], set as lm_set_activation
                          does; with d_goal [n_envs][ngoal] the goal set as lm_set_goal does.
     ls_restart_device    for every masked environment the restart the step kernel performs when an episode ends under
                          lm_set_auto_reset (the reference's trajectory.py:236-273 + base.py:478-497), on request: the episode count
                          advances by one, the reset-table row is drawn from (seed, global environment id, episode count) exactly as
                          there, qpos / qvel / goal come from the row, warm start, activations, slack, episode step and prediction
                          mark are cleared, the model variant is redrawn (a pool: the row's block under lm_set_variant_rows, else a
                          draw of its own; the model compiler: a fresh model, compiled behind the kernel on the same stream,
                          base.py:183-185) and so are the joint parameters under lm_set_dof_randomization. Needs lm_set_reset_table
                          (seed and offset are the table's); lm_set_auto_reset need not be enabled.
   Both writers also store the OBSERVATION ROW of the new state, for the masked environments only: qpos / qvel at their columns,
   the goal columns, the foot-force columns 0 (a fresh running mean, base.py:596-599) — into d_obs [n_envs][nobs], or into the batch's
   own row when d_obs is NULL: the convention of lm_step_device, so lm_rollout_policy with d_obs0 = NULL is valid behind either (behind
   lm_set_state it is not).
   NOT touched by any of the three: the convex collider's warm-start cache, the validity flags, the reward and done rows of the last
   step, the batch's count of control steps (which keys lm_rollout's random actions), the statistics of lm_get_stats — a restart on
   request is not counted as an episode — and the terminal observations. ls_set_state_device leaves the episode count as well.
   Refused with a message, before anything is launched and with nothing changed: a NULL batch; ls_get_state_device with every
   output NULL; ls_set_state_device without d_qpos or d_qvel; d_act for a model without activation states; ls_restart_device
   without a reset table.
   `stream`, `sync`: as in lm_snapshot_save — the launch is ordered behind everything the batch has in flight (the library's stream,
   the replay kernel's pollers, launches on a caller's stream), the library's stream behind it; sync = 0 waits for nothing on the host. */
int ls_get_state_device(lm_batch* b, float* d_qpos, float* d_qvel, float* d_act, float* d_goal,
                        int32_t* d_ep_step, uint32_t* d_ep_count, void* stream, int sync);
int ls_set_state_device(lm_batch* b, const float* d_qpos, const float* d_qvel, const float* d_act, const float* d_goal,
                        const uint8_t* d_mask, float* d_obs, void* stream, int sync);
int ls_restart_device(lm_batch* b, const uint8_t* d_mask, float* d_obs, void* stream, int sync);

#ifdef __cplusplus
}
#endif
#endif
