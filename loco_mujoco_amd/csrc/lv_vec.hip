// lv_vec.hip — the C-ABI (include/locovec.h) of the vector environment's per-step bookkeeping: the done byte taken apart, the observation
// every finished episode ended in, running returns and lengths — one launch behind the step kernel. It reads what a step wrote: no
// lm_batch, no model, no step kernel, and a library of its own (liblocovec.so). Built with -ffp-contract=off and IEEE arithmetic: the
// one addition below is rounded where it is written.
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/locovec.h"

namespace {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return 1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
}  // namespace

namespace lv {
constexpr int kBlock = 256;                 // lanes per workgroup = environments per workgroup

struct FinArgs {
  const float *obs, *reward; const unsigned char* done; const float* term;
  unsigned char *terminated, *truncated; float* final_obs;
  float* run_return; int* run_length; float* ep_return; int* ep_length;
  long long N; int nobs;
};

// A workgroup owns 256 consecutive environments. First the scalars, one lane per environment (every [n] array read and written
// coalesced); then the rows of its environments that ended: [n][nobs] is row-major, so the workgroup's rows are ONE contiguous range of
// floats, which the lanes walk with consecutive lanes on consecutive addresses — whatever nobs is. The done bytes go through LDS, so
// that the walk reads no byte from memory again. Every output element has exactly one writer and takes a value of its own environment
// alone: nothing depends on n_envs, on the environment's place or on the launch shape.
__global__ __launch_bounds__(kBlock) void finish_kernel(FinArgs a) {
  __shared__ unsigned char s_done[kBlock];
  const long long base = (long long)blockIdx.x * kBlock;
  const long long e = base + threadIdx.x;
  unsigned char d = 0;
  if (e < a.N) {
    d = a.done[e];
    a.terminated[e] = (unsigned char)(d & 1);
    a.truncated[e] = (unsigned char)(((d & 2) != 0 && (d & 1) == 0) ? 1 : 0);
    if (a.run_return) {                     // (the host refuses one accumulator without the other)
      float ret = a.run_return[e] + a.reward[e];
      int len = a.run_length[e] + 1;
      float ep_r = 0.0f;
      int ep_l = 0;
      if (d != 0) {
        ep_r = ret; ep_l = len;
        ret = 0.0f; len = 0;                // assigned, not multiplied: a NaN ends with its episode
      }
      a.run_return[e] = ret;
      a.run_length[e] = len;
      if (a.ep_return) a.ep_return[e] = ep_r;
      if (a.ep_length) a.ep_length[e] = ep_l;
    }
  }
  if (!a.final_obs) return;                 // (uniform: a kernel argument)
  s_done[threadIdx.x] = d;                  // lanes past the batch: 0, their rows are never walked
  if (!__syncthreads_or(d != 0)) return;    // (uniform: the barrier's result) most steps end no episode of the workgroup
  const long long rows = a.N - base < kBlock ? a.N - base : kBlock;
  const long long count = rows * a.nobs, first = base * a.nobs;
  for (long long i = threadIdx.x; i < count; i += kBlock) {
    const unsigned char dr = s_done[i / a.nobs];
    if (dr != 0) a.final_obs[first + i] = ((dr & 2) != 0 && a.term ? a.term : a.obs)[first + i];
  }
}

// the grid is ceil(n_envs / 256) workgroups in x
constexpr long long kMaxEnvs = 0x7FFFFFFFLL * kBlock;
}  // namespace lv

extern "C" {

const char* lv_last_error(void) { return g_err.c_str(); }

int lv_finish_step(long long n_envs, int nobs,
                   const float* d_obs, const float* d_reward, const uint8_t* d_done, const float* d_term,
                   uint8_t* d_terminated, uint8_t* d_truncated, float* d_final_obs,
                   float* d_run_return, int32_t* d_run_length, float* d_ep_return, int32_t* d_ep_length,
                   void* stream, int sync) {
  // every argument is checked before the first HIP call: a refused call launches nothing, with or without a device
  if (n_envs < 1 || n_envs > lv::kMaxEnvs) return fail("lv_finish_step: n_envs must be >= 1 (and at most 2^31 - 1 workgroups of 256)");
  if (nobs < 1) return fail("lv_finish_step: nobs must be >= 1");
  if (!d_obs) return fail("lv_finish_step: d_obs is null");
  if (!d_reward) return fail("lv_finish_step: d_reward is null");
  if (!d_done) return fail("lv_finish_step: d_done is null");
  if (!d_terminated) return fail("lv_finish_step: d_terminated is null");
  if (!d_truncated) return fail("lv_finish_step: d_truncated is null");
  if (!d_run_return != !d_run_length) return fail("lv_finish_step: d_run_return and d_run_length are given together or not at all");
  if (d_ep_return && !d_run_return) return fail("lv_finish_step: d_ep_return needs the accumulators d_run_return and d_run_length");
  if (d_ep_length && !d_run_return) return fail("lv_finish_step: d_ep_length needs the accumulators d_run_return and d_run_length");
  if (d_final_obs && d_final_obs == d_obs) return fail("lv_finish_step: d_final_obs must not be d_obs");
  if (d_final_obs && d_final_obs == d_term) return fail("lv_finish_step: d_final_obs must not be d_term");
  const lv::FinArgs a = {d_obs, d_reward, d_done, d_term, d_terminated, d_truncated, d_final_obs,
                         d_run_return, d_run_length, d_ep_return, d_ep_length, n_envs, nobs};
  hipStream_t s = (hipStream_t)stream;
  // the per-thread HIP error state is shared with whoever else uses HIP in this process: what they left behind is dropped, so that
  // the check after the launch reports OURS
  (void)hipGetLastError();
  hipLaunchKernelGGL(lv::finish_kernel, dim3((unsigned)((n_envs + lv::kBlock - 1) / lv::kBlock)), dim3(lv::kBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  if (sync) HIPCHK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
