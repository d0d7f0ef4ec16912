/*
 * locovec.h — C-ABI of the vector environment's per-step bookkeeping ("liblocovec.so"): what a learner does with the outputs of ONE
 * control step (lm_step_device, include/locohip.h) before it may use them — take the done byte apart, pick the observation each finished
 * episode ended in, keep every environment's running return and length — as ONE launch behind the step kernel, on the same stream.
 *
 *   lv_finish_step   <- gymnasium.vector.VectorEnv.step in SAME_STEP autoreset mode: (terminated, truncated), info["final_obs"] and the
 *                       episode statistics of gymnasium's RecordEpisodeStatistics ("episode": {"r", "l"}), per environment
 *
 * This library knows no lm_batch, no model and no step kernel: it reads what a step wrote. All pointers are DEVICE pointers. Functions
 * return 0 on success, non-zero on error; lv_last_error() returns a message for the calling thread. The launch goes to the calling
 * thread's current device (hipSetDevice), which must be the one the buffers and the stream live on.
 */
#ifndef LOCOVEC_H
#define LOCOVEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per calling thread, as lt_last_error */
const char* lv_last_error(void);

/* The bookkeeping of one control step, for environment e with d = d_done[e] (the bit field of lm_step_device: 1 absorbing state, 2 the
   episode ended on the device in this step — restarted from the reset table, or the horizon was reached):
     terminated[e] = d & 1                     (0 / 1)
     truncated[e]  = (d & 2) && !(d & 1)       (0 / 1: an episode that ended without an absorbing state)
     ended         = d != 0
   with the accumulators (caller-owned, both or neither; zero them where a host-side reset drops running episodes):
     run_return[e] = run_return[e] + reward[e]          float32, one rounding
     run_length[e] = run_length[e] + 1
     if ended:  ep_return[e] = run_return[e]; ep_length[e] = run_length[e]
                run_return[e] = 0; run_length[e] = 0    by ASSIGNMENT, never by multiplying with a mask: a NaN reward does not cross an
                                                        episode end
     else:      ep_return[e] = 0; ep_length[e] = 0      (d_ep_return / d_ep_length, each may be NULL, are written for EVERY environment
                                                        in every call)
   and d_final_obs [n_envs][nobs] or NULL, the observation each finished episode ended in:
     a row is written only where ended; it takes d_term[e] where d & 2 and d_term is given (the terminal-observation buffer of
     lm_set_terminal_obs: the step's d_obs row is then the first observation of the NEW episode), and d_obs[e] otherwise (an absorbing
     state without a device-side restart is its own terminal observation). Rows of environments whose episode goes on are NOT touched.
   One launch on `stream` (NULL: the device's null stream; there is no library stream here), no atomics. The scalars are done by one lane
   per environment, the row copies by consecutive lanes on consecutive columns. No value depends on n_envs, on the environment's place in
   the batch or on the launch shape. `sync`: as in lt_tape_episodes (non-zero: hipStreamSynchronize before returning). The caller
   orders the call behind the step that wrote d_obs / d_reward / d_done / d_term, exactly as for a torch op on them.
   Every argument is checked before the first HIP call, so a refusal works on a machine without a GPU, and a refused call launches
   nothing: n_envs < 1, nobs < 1, null d_obs / d_reward / d_done / d_terminated / d_truncated, one accumulator without the other,
   d_ep_return / d_ep_length without the accumulators, d_final_obs equal to d_obs or d_term. */
int lv_finish_step(long long n_envs, int nobs,
                   const float* d_obs, const float* d_reward, const uint8_t* d_done, const float* d_term,
                   uint8_t* d_terminated, uint8_t* d_truncated, float* d_final_obs,
                   float* d_run_return, int32_t* d_run_length, float* d_ep_return, int32_t* d_ep_length,
                   void* stream, int sync);

#ifdef __cplusplus
}
#endif
#endif
