// lm_state_io.h — the state of a batch's environments read, set and restarted from DEVICE memory (include/locostate.h ls_get_state_device,
// ls_set_state_device, ls_restart_device): three kernels, one launch each, and the per-unit work behind them in plain C++ for host and
// device (tests/state_io_main.cpp runs it on the host under the address and undefined-behaviour sanitizers against naive loops).
//
//   gather   one unit per element of qpos / qvel [nv][N], act [na][N], goal [ngoal][N], ep_step / ep_count [N]: consecutive units =
//            consecutive environments of one SoA row (coalesced loads), stored into the caller's row-major [N][dim] buffers
//   scatter  one unit per environment: what lm_set_state / lm_set_activation / lm_set_goal do for it, from the caller's device rows,
//            and the observation row of the new state
//   restart  one unit per environment: the restart block of step_kernel (lm_step.h, under `if (absorbing || trunc)`), restated: the
//            same keys, the same draws, the same float32 expressions — and the same observation row. One unit per environment and
//            not per element: the unit reads ep_count[e] and writes it back, and no other unit may read it in between
//
// A mask byte of 0 yields no operation: nothing of that environment is read or written. No LDS, no tiling: at 4096 environments the
// whole state is 4096 x 35 floats.
#ifndef LM_STATE_IO_H
#define LM_STATE_IO_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LMIO_HD __host__ __device__
#else
#define LMIO_HD
#endif

namespace lmio {

// lm_step.h's mix64, restated (a copy and not a shared header: lm_step.h stays what it is — the precedent is the TERM store there)
LMIO_HD inline unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the batch's arrays these kernels touch (lm_kernels.hip struct lm_batch) and the model's observation maps
struct State {
  int N, nv, na, ngoal, nobs, ngrf;
  float *qpos, *qvel, *warm;      // [nv][N]
  float* act;                     // [na][N], or null
  float* goal;                    // [ngoal][N]
  float* slack;                   // [12][N]
  int* ep_step; unsigned* ep_count; int* premark;      // [N]
  const int *qobs, *vobs;         // [nv]: observation column of qpos[d] / qvel[d], -1: not observed (lm_model_parse.h)
};

// ---- gather
struct GatherArgs {
  State s;
  float *qpos, *qvel, *act, *goal; int32_t* ep_step; uint32_t* ep_count;      // the caller's [N][dim] / [N] buffers, each optional
};
LMIO_HD inline long long gather_units(const State& s) { return (long long)s.N * (2 * s.nv + s.na + s.ngoal + 2); }

LMIO_HD inline void gather_unit(const GatherArgs& a, long long u) {
  const State& s = a.s;
  const long long N = s.N;
  if (u < 0 || u >= gather_units(s)) return;
  long long row = u / N;
  const long long e = u - row * N;
  if (row < s.nv) { if (a.qpos) a.qpos[e * s.nv + row] = s.qpos[row * N + e]; return; }
  row -= s.nv;
  if (row < s.nv) { if (a.qvel) a.qvel[e * s.nv + row] = s.qvel[row * N + e]; return; }
  row -= s.nv;
  if (row < s.na) { if (a.act && s.act) a.act[e * s.na + row] = s.act[row * N + e]; return; }
  row -= s.na;
  if (row < s.ngoal) { if (a.goal) a.goal[e * s.ngoal + row] = s.goal[row * N + e]; return; }
  row -= s.ngoal;
  if (row == 0) { if (a.ep_step) a.ep_step[e] = s.ep_step[e]; }
  else if (a.ep_count) a.ep_count[e] = s.ep_count[e];
}

// the observation row of a fresh state, as the step kernel stores it: [qpos[d] at qobs[d] | qvel[d] at vobs[d] | goal | foot forces 0]
LMIO_HD inline void store_obs_dof(const State& s, float* o, int d, float q, float v) {
  const int iq = s.qobs[d], iv = s.vobs[d];      // (inside the row or -1: lm_model_parse.h maps every other column to -1)
  if (iq >= 0) o[iq] = q;
  if (iv >= 0) o[iv] = v;
}
LMIO_HD inline void store_obs_grf(const State& s, float* o) {
  for (int i = 0; i < s.ngrf; i++) o[s.nobs - s.ngrf + i] = 0.0f;      // a fresh running mean
}
// what a new state voids: solver warm start, the self-collision pass's slack, the episode's step, the replay prediction
LMIO_HD inline void clear_env(const State& s, int e, bool zero_act) {
  const long long N = s.N;
  for (int d = 0; d < s.nv; d++) s.warm[d * N + e] = 0.0f;
  if (zero_act && s.act) for (int i = 0; i < s.na; i++) s.act[i * N + e] = 0.0f;
  for (int j = 0; j < 12; j++) s.slack[j * N + e] = 0.0f;
  s.ep_step[e] = 0;
  s.premark[e] = 0;
}

// ---- scatter
struct ScatterArgs {
  State s;
  const float *qpos, *qvel;       // [N][nv]
  const float* act;               // [N][na], or null: activations are zeroed
  const float* goal;              // [N][ngoal], or null: the goal stays
  const uint8_t* mask;            // [N], or null: all
  float* obs;                     // [N][nobs]: where the observation rows go
};

LMIO_HD inline void scatter_env(const ScatterArgs& a, int e) {
  const State& s = a.s;
  if (e < 0 || e >= s.N || (a.mask && !a.mask[e])) return;
  const long long N = s.N;
  float* o = a.obs + (long long)e * s.nobs;
  for (int d = 0; d < s.nv; d++) {
    const float q = a.qpos[(long long)e * s.nv + d], v = a.qvel[(long long)e * s.nv + d];
    s.qpos[d * N + e] = q; s.qvel[d * N + e] = v;
    store_obs_dof(s, o, d, q, v);
  }
  clear_env(s, e, a.act == nullptr);
  if (a.act && s.act) for (int i = 0; i < s.na; i++) s.act[i * N + e] = a.act[(long long)e * s.na + i];
  for (int i = 0; i < s.ngoal; i++) {
    const float g = a.goal ? a.goal[(long long)e * s.ngoal + i] : s.goal[i * N + e];
    if (a.goal) s.goal[i * N + e] = g;
    o[s.nobs - s.ngrf - s.ngoal + i] = g;
  }
  store_obs_grf(s, o);
}

// ---- restart
struct RestartArgs {
  State s;
  const float* table; int table_rows;      // [table_rows][2 nv + ngoal]
  unsigned long long seed; long long env_offset;
  unsigned char* vdirty;          // the model compiler's restart flags [N], or null
  int* var; int nvar, var_rows;   // the variant pool's index [N] (lm_step.h KArgs::var)
  float* dofprm;                  // [3][nv][N], or null
  const float* drspec;            // [3][nv][3] = (kind, a, b), or null
  const uint8_t* mask;
  float* obs;
};

// the key of (environment, episode): lm_step.h's seed ^ mix64(gid * 2 + 1) ^ (ec << 32)
LMIO_HD inline unsigned long long episode_key(unsigned long long seed, long long gid, unsigned ec) {
  return seed ^ mix64((unsigned long long)gid * 2ull + 1ull) ^ ((unsigned long long)ec << 32);
}
LMIO_HD inline long long restart_row(unsigned long long seed, long long gid, unsigned ec, int table_rows) {
  return (long long)(mix64(episode_key(seed, gid, ec)) % (unsigned long long)table_rows);
}
// a joint parameter redrawn with the episode: the keys and the float32 expressions of the step kernel's `redraw` lambda
LMIO_HD inline float redraw_value(unsigned long long key, int dof, int p, int kind, float sa, float sb) {
  const unsigned long long r = mix64(key ^ (unsigned long long)(dof * 3 + p + 1) * 0xD6E8FEB86659FD93ull);
  const float u1 = ((float)(r >> 40) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)((r >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
  if (kind == 2) return sa + (sb - sa) * u1;                          // U(a, b)
  const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);    // N(a, b)
  return fmaxf(fmaf(sb, z, sa), 0.0f);      // both normal kinds are clipped at 0 (a joint parameter cannot be negative)
}

LMIO_HD inline void restart_env(const RestartArgs& a, int e) {
  const State& s = a.s;
  if (e < 0 || e >= s.N || (a.mask && !a.mask[e])) return;      // (table_rows >= 1: ls_restart_device refuses a batch without a table)
  const long long N = s.N, gid = a.env_offset + e;
  const int nv = s.nv;
  const unsigned ec = s.ep_count[e] + 1;
  const unsigned long long key = episode_key(a.seed, gid, ec);
  const long long drawn = restart_row(a.seed, gid, ec, a.table_rows);
  const float* row = a.table + drawn * (2 * nv + s.ngoal);
  float* o = a.obs + (long long)e * s.nobs;
  for (int d = 0; d < nv; d++) {
    const float q = row[d], v = row[nv + d];
    s.qpos[d * N + e] = q; s.qvel[d * N + e] = v;
    store_obs_dof(s, o, d, q, v);
  }
  for (int i = 0; i < s.ngoal; i++) {
    const float g = row[2 * nv + i];
    s.goal[i * N + e] = g;
    o[s.nobs - s.ngrf - s.ngoal + i] = g;
  }
  store_obs_grf(s, o);
  clear_env(s, e, true);
  s.ep_count[e] = ec;
  // new episode, new model: the compiler's flag, or the pool's index — the block of the row drawn above, or a draw of its own
  if (a.vdirty) a.vdirty[e] = 1;
  else if (a.nvar > 1 && a.var)
    a.var[e] = a.var_rows > 0 ? (int)(drawn / a.var_rows) : (int)(mix64(key ^ 0xA24BAED4963EE407ull) % (unsigned long long)a.nvar);
  if (a.dofprm && a.drspec)
    for (int p = 0; p < 3; p++)
      for (int d = 0; d < nv; d++) {
        const float* sp = a.drspec + ((long long)p * nv + d) * 3;
        const int kind = (int)sp[0];
        if (kind != 0) a.dofprm[((long long)p * nv + d) * N + e] = redraw_value(key, d, p, kind, sp[1], sp[2]);
      }
}

#if defined(__HIPCC__)
constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) state_gather_kernel(const GatherArgs a) {
  const long long total = gather_units(a.s), stride = (long long)gridDim.x * kThreads;
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < total; u += stride) gather_unit(a, u);
}
__global__ void __launch_bounds__(kThreads) state_scatter_kernel(const ScatterArgs a) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e < a.s.N) scatter_env(a, (int)e);
}
__global__ void __launch_bounds__(kThreads) restart_kernel(const RestartArgs a) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e < a.s.N) restart_env(a, (int)e);
}

inline unsigned env_blocks(int N) { return (unsigned)((N + kThreads - 1) / kThreads); }
inline void launch_gather(const GatherArgs& a, hipStream_t stream) {
  long long blocks = (gather_units(a.s) + kThreads - 1) / kThreads;
  if (blocks > 4096) blocks = 4096;      // grid-stride beyond that, as lm_snapshot.h
  if (blocks > 0) hipLaunchKernelGGL(state_gather_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
}
inline void launch_scatter(const ScatterArgs& a, hipStream_t stream) {
  if (a.s.N > 0) hipLaunchKernelGGL(state_scatter_kernel, dim3(env_blocks(a.s.N)), dim3(kThreads), 0, stream, a);
}
inline void launch_restart(const RestartArgs& a, hipStream_t stream) {
  if (a.s.N > 0) hipLaunchKernelGGL(restart_kernel, dim3(env_blocks(a.s.N)), dim3(kThreads), 0, stream, a);
}
#endif

}  // namespace lmio
#endif
