// lm_policy.h — a small MLP policy evaluated on the device, for closed-loop rollouts (include/locohip.h lm_rollout_policy).
//
// policy_row() is THE evaluation: called by the 16 lanes that own an environment (a row of a wave: threadIdx.x & 15 = the lane's
// number among them), it reads the observation row [nobs] and the caller's parameters in place and writes the action row [nu].
// Lane l computes the units j = l (mod 16) of every layer; a unit accumulates in float32 in ONE order — its bias first, then the
// inputs in index order, one fmaf each — and the activations, the noise and the final a = mean + std * z are spelled out in single
// operations and explicit fmaf calls, so that -ffp-contract has nothing to decide: an action does not depend on which kernel,
// workgroup or batch computed it, nor on how many of a unit's neighbours the lane computes beside it.
//
// Hidden activations pass between the lanes through a hand-over buffer `h` of 2 * kPolicyMaxWidth floats that the caller provides per
// environment. policy_kernel (lm_kernels.hip): LDS of its own, 2 KB per environment (it is no step kernel, lm_lds_bytes does not count it) — the 16
// lanes sit in one wave and run in lock step, and the LDS executes a wave's instructions in order: the hand-over needs a
// compiler-level fence only, as the replicas' hand-over in lm_step.h (QuadDppT::fence). The POLICY instantiations of the fused step
// kernels (GLOBAL_HAND): a row per environment in global memory and the agent-scope fence with which the lanes of an environment
// already hand their state from one fused control step to the next — the step kernels' LDS stays what lm_lds_bytes reports, and the
// replay kernels, whose lane memory is the whole LDS a workgroup can have, need no room for it. The arithmetic is the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/locohip.h"

namespace lmp {

constexpr int kPolicyMaxWidth = 256;     // hidden widths 1..256 (locohip.h lm_mlp_policy)
constexpr int kPolicyMaxLayers = 3;
// the salt of the action noise: the uniform actions of the step kernel (action_mode 2) use the same key without it, the restart
// draws key by the episode count — no two of the three streams share a number under one seed
constexpr unsigned long long kPolicyNoiseSalt = 0x5851F42D4C957F2Dull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {      // (the step kernel's counter hash, lm_step.h)
  x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// a value the optimiser cannot see through: the products and library results below are not contracted into their neighbours' additions
// (-ffp-contract=fast), whatever code surrounds the call
__device__ __forceinline__ float policy_opaque(float x) { asm volatile("" : "+v"(x)); return x; }

// n / d to within an ulp whatever the build's division flags are: v_rcp_f32 and two residual corrections, every step an fmaf
__device__ __forceinline__ float policy_div(float n, float d) {
  float r = __builtin_amdgcn_rcpf(d);
  r = fmaf(fmaf(-d, r, 1.0f), r, r);
  const float q = n * r;
  return fmaf(fmaf(-d, q, n), r, q);
}
// tanh(x) = -m / (m + 2), m = expm1(-2 |x|): no cancellation near 0, saturates to 1 without overflow
__device__ __forceinline__ float policy_tanh(float x) {
  const float m = policy_opaque(expm1f(policy_opaque(-2.0f * fabsf(x))));
  return copysignf(policy_div(-m, m + 2.0f), x);
}

// one unit group of a layer: the units j0, j0 + 16, j0 + 32, j0 + 48 of lane j0 & 15 side by side (four independent chains of fmaf:
// the loads of one hide behind the others), each in its own fixed order
__device__ __forceinline__ void policy_units(const float* __restrict__ W, const float* __restrict__ bias, const float* x, int n_in, int n_out, int j0,
                                             float* y, bool hidden, int activation) {
  int j[4]; float acc[4]; const float* w[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    j[t] = j0 + 16 * t;
    const int jj = j[t] < n_out ? j[t] : n_out - 1;      // (a unit beyond the layer: recompute the last one, store nothing)
    w[t] = W + (long long)jj * n_in; acc[t] = bias[jj];
  }
#pragma unroll 4
  for (int i = 0; i < n_in; i++) {
    const float xi = x[i];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = fmaf(w[t][i], xi, acc[t]);
  }
#pragma unroll
  for (int t = 0; t < 4; t++) {
    float v = acc[t];
    if (hidden) v = activation == 0 ? policy_tanh(v) : fmaxf(v, 0.0f);
    if (j[t] < n_out) y[j[t]] = v;
  }
}

// INPUT NORMALISATION (locohip.h lm_set_policy_obs_norm): what the first layer reads is clamp((obs - mean) * inv_std, -clip, clip), the
// running standardiser in front of a locomotion actor. mean / inv_std: the caller's device tensors [nobs] in the kernel's column order,
// read in place at every evaluation like the parameters; mean null: off — the load below is then the plain copy it was. One subtraction,
// one multiplication and two selects, each a single rounding of its own (nothing here can contract; the product is made opaque all the
// same, so that the selects stay selects whatever surrounds the call): torch's ((x - mean) * inv_std).clamp(-clip, clip) bit for bit,
// a NaN staying NaN. clip == 0: no clamp. Only the policy's input is normalised: the observation row itself stays as the step wrote it.
struct PolicyNorm { const float* mean; const float* inv_std; float clip; };

template <bool GLOBAL_HAND>
__device__ __forceinline__ void policy_handover() {
  if (GLOBAL_HAND) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The action row of ONE environment, by its 16 lanes (lane = 0..15). obs [nobs] and act [nu] are the environment's rows; h: the
// hand-over buffer [2][kPolicyMaxWidth] of this environment. gid = the GLOBAL environment id, step = the batch's count of control
// steps at this step: with p.d_log_std the key of the noise (noise_seed, gid, step, k).
template <bool GLOBAL_HAND = false>
__device__ __forceinline__ void policy_row(const lm_mlp_policy& p, const PolicyNorm& nrm, const float* __restrict__ obs, float* __restrict__ act, float* h, int lane,
                                           unsigned long long noise_seed, long long gid, unsigned step) {
  float* x = h; float* y = h + kPolicyMaxWidth;
  if (nrm.mean) {
    const float clip = nrm.clip;
    for (int i = lane; i < p.sizes[0]; i += 16) {
      const float d = policy_opaque(obs[i] - nrm.mean[i]);
      const float t = policy_opaque(d * nrm.inv_std[i]);
      x[i] = clip > 0.0f ? (t < -clip ? -clip : (t > clip ? clip : t)) : t;
    }
  } else {
    for (int i = lane; i < p.sizes[0]; i += 16) x[i] = obs[i];
  }
  policy_handover<GLOBAL_HAND>();
  const float* prm = p.d_params;
  for (int l = 0; l < p.n_layers; l++) {
    const int n_in = p.sizes[l], n_out = p.sizes[l + 1];
    const float* W = prm; const float* bias = prm + (long long)n_in * n_out;
    prm = bias + n_out;
    const bool last = l == p.n_layers - 1;
    for (int j0 = lane; j0 < n_out; j0 += 64) policy_units(W, bias, x, n_in, n_out, j0, y, !last, p.activation);
    policy_handover<GLOBAL_HAND>();
    float* t = x; x = y; y = t;
  }
  // x: the mean [nu]
  for (int k = lane; k < p.sizes[p.n_layers]; k += 16) {
    float a = x[k];
    if (p.d_log_std) {
      const unsigned long long r = mix64(noise_seed ^ mix64((unsigned long long)gid * 0x100000001B3ull + step) ^ (unsigned long long)(k + 1) * 0xD6E8FEB86659FD93ull ^ kPolicyNoiseSalt);
      const float u1 = ((float)(r >> 40) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)((r >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
      const float rad = policy_opaque(sqrtf(policy_opaque(-2.0f * policy_opaque(logf(u1)))));
      const float z = policy_opaque(rad * policy_opaque(cosf(policy_opaque(6.2831853f * u2))));       // Box-Muller
      a = fmaf(policy_opaque(expf(p.d_log_std[k])), z, a);
    }
    act[k] = a;
  }
}

}  // namespace lmp
