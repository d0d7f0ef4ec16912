// lt_tapes.hip — the C-ABI (include/locotape.h) of the learner's side of the tapes: episode returns, lengths and the running discounted
// return from the reward and done tapes, carried across rollouts. Tapes only: no lm_batch, no model, no step kernel, and a library of
// its own (liblocotape.so). Built with -ffp-contract=off and IEEE division: every operation below is rounded where it is written.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "../../include/locotape.h"

namespace {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return 1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
}  // namespace

namespace lt {
constexpr int kBlock = 256;                 // lanes per workgroup: the unit of the summary's fixed tree and of d_work
// the fields of the summary (locotape.h LT_SUMMARY_FIELDS), in order
enum { S_EPISODES, S_R, S_RR, S_RMIN, S_RMAX, S_J, S_L, S_LMIN, S_LMAX, S_ABSORBING, S_FIELDS };
static_assert(S_FIELDS == LT_SUMMARY_FIELDS, "the summary's fields");

__host__ __device__ inline long long n_blocks(long long n) { return (n + kBlock - 1) / kBlock; }
__device__ inline double identity(int f) {
  return (f == S_RMIN || f == S_LMIN) ? __builtin_huge_val() : (f == S_RMAX || f == S_LMAX) ? -__builtin_huge_val() : 0.0;
}
// a (+) b of field f: a sum, or a min / max that passes over a NaN in b (a never holds one: it starts from the identity)
__device__ inline double combine(int f, double a, double b) {
  if (f == S_RMIN || f == S_LMIN) return b < a ? b : a;
  if (f == S_RMAX || f == S_LMAX) return b > a ? b : a;
  return a + b;
}

struct EpArgs {
  const float* reward; const unsigned char *done, *mask; float gamma;
  float* carry; int* len;
  float *ep_return, *ep_disc; int* ep_length; float* trace;
  double* work; int T; long long N;
};

// One environment per lane, so that every row [t][.] of a tape is read and written coalesced; t ascending with the carry in registers.
// Every lane of the workgroup reaches the tree below, with the identity where it has no environment or a masked one: the tree's shape
// depends on n_envs alone.
__global__ __launch_bounds__(kBlock) void episodes_kernel(EpArgs a) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool on = e < a.N && (!a.mask || a.mask[e] != 0);
  double p[S_FIELDS];
#pragma unroll
  for (int f = 0; f < S_FIELDS; f++) p[f] = identity(f);
  if (on) {
    float ret = a.carry[e], disc = a.carry[a.N + e], w = a.carry[2 * a.N + e], g = a.carry[3 * a.N + e];
    int len = a.len[e];
    for (int t = 0; t < a.T; t++) {
      const long long at = (long long)t * a.N + e;
      const float r = a.reward[at];
      const unsigned char d = a.done[at];
      ret = ret + r;
      disc = fmaf(w, r, disc);
      w = w * a.gamma;
      g = fmaf(a.gamma, g, r);
      len = len + 1;
      if (a.trace) a.trace[at] = g;
      if (d != 0) {
        if (a.ep_return) a.ep_return[at] = ret;
        if (a.ep_disc) a.ep_disc[at] = disc;
        if (a.ep_length) a.ep_length[at] = len;
        const double R = (double)ret, J = (double)disc, L = (double)len;
        p[S_EPISODES] = p[S_EPISODES] + 1.0;
        p[S_R] = p[S_R] + R;
        p[S_RR] = p[S_RR] + R * R;
        p[S_RMIN] = combine(S_RMIN, p[S_RMIN], R);
        p[S_RMAX] = combine(S_RMAX, p[S_RMAX], R);
        p[S_J] = p[S_J] + J;
        p[S_L] = p[S_L] + L;
        p[S_LMIN] = combine(S_LMIN, p[S_LMIN], L);
        p[S_LMAX] = combine(S_LMAX, p[S_LMAX], L);
        p[S_ABSORBING] = p[S_ABSORBING] + (double)(d & 1);
        ret = 0.0f; disc = 0.0f; w = 1.0f; g = 0.0f; len = 0;          // assigned, not multiplied: a NaN ends with its episode
      }
    }
    a.carry[e] = ret; a.carry[a.N + e] = disc; a.carry[2 * a.N + e] = w; a.carry[3 * a.N + e] = g;
    a.len[e] = len;
  }
  if (!a.work) return;                      // (uniform: a kernel argument)
  // the fixed tree: lane i takes lane i + s for s = 128, 64 ... 1; field-major rows, so that the lanes of a wave read consecutive doubles
  __shared__ double part[S_FIELDS][kBlock];
  const int i = threadIdx.x;
#pragma unroll
  for (int f = 0; f < S_FIELDS; f++) part[f][i] = p[f];
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (i < s) {
#pragma unroll
      for (int f = 0; f < S_FIELDS; f++) part[f][i] = combine(f, part[f][i], part[f][i + s]);
    }
    __syncthreads();
  }
  if (i < S_FIELDS) a.work[(long long)blockIdx.x * S_FIELDS + i] = part[i][0];
}

// the workgroups' partials in index order, one lane per field; then into the summary: over it, or merged with what it holds
__global__ __launch_bounds__(64) void summary_kernel(const double* work, long long blocks, double* summary, int accumulate) {
  const int f = threadIdx.x;
  if (f >= S_FIELDS) return;
  double acc = identity(f);
  for (long long k = 0; k < blocks; k++) acc = combine(f, acc, work[k * S_FIELDS + f]);
  summary[f] = accumulate ? combine(f, summary[f], acc) : acc;
}

__global__ __launch_bounds__(kBlock) void carry_reset_kernel(float* carry, int* len, const unsigned char* mask, long long N) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= N || (mask && mask[e] == 0)) return;
  carry[e] = 0.0f; carry[N + e] = 0.0f; carry[2 * N + e] = 1.0f; carry[3 * N + e] = 0.0f;
  len[e] = 0;
}

// `queue(stream)` on the caller's stream (null: the device's null stream). The per-thread HIP error state is shared with whoever else
// uses HIP in this process: what they left behind is dropped, so that the check after `queue` reports OUR launches
template <class Queue> static int on_stream(void* stream, int sync, Queue queue) {
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  queue(s);
  HIPCHK(hipGetLastError());
  if (sync) HIPCHK(hipStreamSynchronize(s));
  return 0;
}
// the grid is ceil(n_envs / 256) workgroups in x
constexpr long long kMaxEnvs = 0x7FFFFFFFLL * kBlock;
}  // namespace lt

extern "C" {

const char* lt_last_error(void) { return g_err.c_str(); }

long long lt_episode_work_doubles(long long n_envs) { return n_envs < 1 ? 0 : lt::n_blocks(n_envs) * LT_SUMMARY_FIELDS; }

int lt_episode_carry_reset(long long n_envs, float* d_carry, int32_t* d_len, const uint8_t* d_mask, void* stream, int sync) {
  if (n_envs < 1 || n_envs > lt::kMaxEnvs) return fail("lt_episode_carry_reset: n_envs must be >= 1 (and at most 2^31 - 1 workgroups of 256)");
  if (!d_carry) return fail("lt_episode_carry_reset: d_carry is null");
  if (!d_len) return fail("lt_episode_carry_reset: d_len is null");
  return lt::on_stream(stream, sync, [&](hipStream_t s) {
    hipLaunchKernelGGL(lt::carry_reset_kernel, dim3((unsigned)lt::n_blocks(n_envs)), dim3(lt::kBlock), 0, s, d_carry, d_len, d_mask, n_envs);
  });
}

int lt_tape_episodes(int n_steps, long long n_envs, const float* d_reward, const uint8_t* d_done, const uint8_t* d_mask, float gamma,
                     float* d_carry, int32_t* d_len,
                     float* d_ep_return, float* d_ep_disc_return, int32_t* d_ep_length, float* d_return_trace,
                     double* d_summary, int accumulate, double* d_work, void* stream, int sync) {
  // every argument is checked before the first HIP call: a refused call launches nothing, with or without a device
  if (n_steps < 1) return fail("lt_tape_episodes: n_steps must be >= 1");
  if (n_envs < 1 || n_envs > lt::kMaxEnvs) return fail("lt_tape_episodes: n_envs must be >= 1 (and at most 2^31 - 1 workgroups of 256)");
  if (!d_reward) return fail("lt_tape_episodes: d_reward is null");
  if (!d_done) return fail("lt_tape_episodes: d_done is null");
  if (!d_carry) return fail("lt_tape_episodes: d_carry is null");
  if (!d_len) return fail("lt_tape_episodes: d_len is null");
  if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail("lt_tape_episodes: gamma must be in [0, 1]");
  if (d_summary && !d_work) return fail("lt_tape_episodes: d_summary needs d_work (lt_episode_work_doubles(n_envs) doubles)");
  const long long blocks = lt::n_blocks(n_envs);
  const lt::EpArgs a = {d_reward, d_done, d_mask, gamma, d_carry, d_len, d_ep_return, d_ep_disc_return, d_ep_length, d_return_trace,
                        d_summary ? d_work : nullptr, n_steps, n_envs};
  return lt::on_stream(stream, sync, [&](hipStream_t s) {
    hipLaunchKernelGGL(lt::episodes_kernel, dim3((unsigned)blocks), dim3(lt::kBlock), 0, s, a);
    // a launch of its own behind the first: every workgroup's partial is in d_work when it starts
    if (d_summary) hipLaunchKernelGGL(lt::summary_kernel, dim3(1), dim3(64), 0, s, (const double*)d_work, blocks, d_summary, accumulate);
  });
}

}  // extern "C"
