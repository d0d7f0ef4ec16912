// lm_model_parse.h — the host side of lm_model_create: an untrusted "chain model" blob (include/lm_layout.h) is checked and turned into task
// facts, scalar parameters and the float tables that go to the device. Plain C++17, no HIP: tests/model_parse_main.cpp runs it under sanitizers.
#pragma once
#include <stddef.h>
#include <string>
#include <vector>
#include "lm_families.h"

namespace lmp {
struct ParsedModel {
  lmk::Task T;
  float h, g[3], scale;      // the scalars of lm::Params (lm_core.h) that the blob sets
  int iterations, integrator, cone, act_position, off_runsup, neq, off_eq;
  bool root_limited;         // a root dof with an active-able limit (lm_batch_set_replay)
  bool root_xyz;             // the root's first three dofs are slides along +x, +y, +z in a root frame that is the world's (lm_core.h ROOT_XYZ)
  std::vector<float> nominal;      // [3][nv] damping | stiffness | frictionloss of the model
  std::vector<int> qobs, vobs;     // [nv] observation column of qpos[d] / qvel[d] (the dof records' LM_D_QOBS / LM_D_VOBS), -1: not observed
  // constant, geom, muscle (empty: no muscles), geom-pair (n_gpt_floats: without its padding), hull-vertex, neighbour, body-pair, adjacency tables
  std::vector<float> cm, gt, mt, gpt, meshv, meshn, bpt, meshadj; int n_gpt_floats;
};
inline bool refuse(std::string* why, const char* msg) { *why = msg; return false; }
// An optional table of `count` records of `rec` doubles at `off` (as the header states them), copied into `out` with `pad` more entries of
// `fill`. false: the blob does not hold it — a count or offset that is negative, not a number or beyond the blob included.
inline bool optional_table(const double* cmod, size_t n, double count, double off, size_t rec, size_t pad, float fill, std::vector<float>* out, size_t* records = nullptr) {
  if (!(count > -1.0 && count <= (double)n)) return false;
  const size_t cnt = (size_t)count * rec;
  if (cnt > 0 && !(off > -1.0 && off <= (double)n && cnt <= n - (size_t)off)) return false;
  const size_t at = cnt > 0 ? (size_t)off : 0;
  out->assign(cnt + pad, fill);
  for (size_t i = 0; i < cnt; i++) (*out)[i] = (float)cmod[at + i];
  if (records) *records = (size_t)count;
  return true;
}

inline bool parse_model(const double* cmod, size_t n, ParsedModel* out, std::string* why) {
  if (!cmod || n < LM_HEADER_SIZE + LM_CM_SIZE + LM_GT_SIZE) return refuse(why, "chain model too short");
  if ((unsigned)cmod[LM_H_MAGIC] != (unsigned)LM_LMC_MAGIC) return refuse(why, "bad chain-model magic");
  if ((int)cmod[LM_H_CM_SIZE] != LM_CM_SIZE || (int)cmod[LM_H_GT_SIZE] != LM_GT_SIZE) return refuse(why, "chain-model table size mismatch (regenerate include/lm_layout.h)");
  if ((int)cmod[LM_H_MAXLINKS] > LM_MAXC) return refuse(why, "chains longer than 7 links are not supported");
  if ((int)cmod[LM_HEADER_SIZE + LM_R_NDOF] != 6) return refuse(why, "root body must have 6 dofs");
  const int n_muscle = (int)cmod[LM_H_NMUSCLE];
  if (n_muscle < 0 || n_muscle > LM_MT_MAXMUS) return refuse(why, "bad muscle count");
  if (n_muscle > 0 && n < (size_t)(LM_HEADER_SIZE + LM_CM_SIZE + LM_GT_SIZE + LM_MT_SIZE)) return refuse(why, "chain model lacks the muscle table");
  if (n_muscle > 0 && (int)cmod[LM_H_INTEGRATOR] != LM_INT_EULER) return refuse(why, "muscles need the Euler integrator");
  ParsedModel& m = *out;
  auto take = [&](size_t at, size_t count, std::vector<float>* v) { v->resize(count); for (size_t i = 0; i < count; i++) (*v)[i] = (float)cmod[at + i]; };
  std::vector<float>& cm = m.cm;
  take(LM_HEADER_SIZE, LM_CM_SIZE, &cm);
  // (limited root joints: limit rows in the muscle families, the run-time-cone kernels and every family's replay kernel; the other
  // regular kernels hand a control step with a root dof beyond its range to the replay kernel — lm_core.h ROOT_LIM)
  m.root_limited = false;
  for (int i = 0; i < 6; i++) if (cm[LM_R_DOFS + i * LM_D_SIZE + LM_D_LIMITED] != 0.0f) m.root_limited = true;
  m.root_xyz = cm[LM_R_NDOF] == 6.0f;
  for (int i = 0; i < 9; i++) if (cm[LM_R_R0 + i] != ((i % 4 == 0) ? 1.0f : 0.0f)) m.root_xyz = false;
  for (int i = 0; i < 3; i++) {
    const float* d = cm.data() + LM_R_DOFS + i * LM_D_SIZE;
    if (d[LM_D_TYPE] != 0.0f) m.root_xyz = false;                       // (0 = slide: mjcf.JNT_SLIDE)
    for (int k = 0; k < 3; k++) if (d[LM_D_AX + k] != ((k == i) ? 1.0f : 0.0f)) m.root_xyz = false;
  }
  take(LM_HEADER_SIZE + LM_CM_SIZE, LM_GT_SIZE, &m.gt);
  take(LM_HEADER_SIZE + LM_CM_SIZE + LM_GT_SIZE, n_muscle > 0 ? LM_MT_SIZE : 0, &m.mt);
  for (int c = 0; c < LM_NCHAIN && n_muscle > 0; c++) if ((int)m.mt[LM_NCHAIN + c] > LM_MAXMUS) return refuse(why, "too many muscles on one chain");
  lmk::Task& T = m.T;
  T.na = n_muscle;
  const int nv = (int)cmod[LM_H_NV];
  m.nominal.assign((size_t)3 * nv, 0.0f);
  m.qobs.assign((size_t)(nv > 0 ? nv : 0), -1); m.vobs.assign((size_t)(nv > 0 ? nv : 0), -1);
  const int nobs_h = (int)cmod[LM_H_NOBS];
  auto put = [&](const float* blk, int stride) {
    const int d = (int)blk[LM_D_DOF * stride];
    if (d < 0 || d >= nv) return;
    m.nominal[d] = blk[LM_D_DAMP * stride]; m.nominal[nv + d] = blk[LM_D_STIFF * stride]; m.nominal[2 * nv + d] = blk[LM_D_FLOSS * stride];
    // (a column outside the observation row counts as not observed: lm_state_io.h writes through these maps)
    const int iq = (int)blk[LM_D_QOBS * stride], iv = (int)blk[LM_D_VOBS * stride];
    m.qobs[d] = (iq >= 0 && iq < nobs_h) ? iq : -1; m.vobs[d] = (iv >= 0 && iv < nobs_h) ? iv : -1;
  };
  for (int i = 0; i < 6; i++) put(cm.data() + LM_R_DOFS + i * LM_D_SIZE, 1);
  for (int c = 0; c < LM_NCHAIN; c++) {
    const int nl = (int)cm[LM_CM_CHAINS + LM_C_NLINKS * LM_NCHAIN + c];
    // (refused: a link count whose last record's dof index, the furthest field read here, lies outside the constant table)
    if (nl > 0 && (size_t)LM_CM_CHAINS + ((size_t)LM_C_LINKS + (size_t)(nl - 1) * LM_LINK_SIZE + LM_D_DOF) * LM_NCHAIN + c >= (size_t)LM_CM_SIZE) return refuse(why, "a chain's link count runs past the constant table");
    for (int k = 0; k < nl; k++) put(cm.data() + LM_CM_CHAINS + (LM_C_LINKS + k * LM_LINK_SIZE) * LM_NCHAIN + c, LM_NCHAIN);
  }
  T.nv = nv; T.nu = (int)cmod[LM_H_NU]; T.nobs = (int)cmod[LM_H_NOBS]; T.ngoal = (int)cmod[LM_H_NGOAL];
  T.nsub = (int)cmod[LM_H_NSUBSTEPS]; T.reward_type = (int)cmod[LM_H_REWARD_TYPE];
  T.n_chains = (int)cmod[LM_H_NCHAINS]; T.max_links = (int)cmod[LM_H_MAXLINKS]; T.ngrf = (int)cmod[LM_H_NGRF];
  T.max_contacts = (int)cmod[LM_H_MAXCONTACTS]; T.npair = (int)cmod[LM_H_NGPAIR];
  // every geom with a device collider is a condim-3 contact under pyramidal cones? (refused: a geom count whose last record lies outside the blob)
  T.all_pyr3 = (int)cmod[LM_H_CONE] == LM_CONE_PYRAMIDAL;
  for (int c = 0; c < LM_NCHAIN && T.all_pyr3; c++) {
    const int ng = (int)cmod[LM_HEADER_SIZE + LM_CM_CHAINS + LM_C_NGEOMS * LM_NCHAIN + c];
    if (ng > 0 && (size_t)LM_HEADER_SIZE + LM_CM_SIZE + ((size_t)(ng - 1) * LM_G_SIZE + LM_G_DIM) * LM_NCHAIN + c >= n) return refuse(why, "a chain's geom count runs past the chain model");
    for (int g = 0; g < ng; g++) if ((int)cmod[LM_HEADER_SIZE + LM_CM_SIZE + (g * LM_G_SIZE + LM_G_DIM) * LM_NCHAIN + c] != 3) T.all_pyr3 = 0;
  }
  T.cm_used = ((int)cmod[LM_H_CM_USED] + 63) & ~63;          // keeps lane memory 256-byte aligned behind the table
  if (T.cm_used <= 0 || T.cm_used > ((LM_CM_SIZE + 63) & ~63)) return refuse(why, "bad constant-table extent");
  if (T.ngoal > 4) return refuse(why, "more than 4 goal entries");
  for (int i = 0; i < 8; i++) T.rp[i] = (float)cmod[LM_H_REWARD_P0 + i];
  m.h = (float)cmod[LM_H_TIMESTEP]; m.g[0] = (float)cmod[LM_H_GX]; m.g[1] = (float)cmod[LM_H_GY]; m.g[2] = (float)cmod[LM_H_GZ]; m.iterations = (int)cmod[LM_H_ITERATIONS];
  m.integrator = (int)cmod[LM_H_INTEGRATOR]; m.cone = (int)cmod[LM_H_CONE]; m.act_position = (int)cmod[LM_H_ACTMODE];
  m.scale = 1.0f / ((float)cmod[LM_H_MEANINERTIA] * (float)T.nv); m.off_runsup = (int)cmod[LM_H_OFF_RUNSUP];
  size_t ngp = 0;
  if (!optional_table(cmod, n, cmod[LM_H_NGPAIR], cmod[LM_H_OFF_GPT], LM_GPAIR_SIZE, 1, 0.0f, &m.gpt, &ngp)) return refuse(why, "chain model lacks the geom-pair table");
  m.n_gpt_floats = (int)(ngp * LM_GPAIR_SIZE);
  if (!optional_table(cmod, n, cmod[LM_H_NMESHV], cmod[LM_H_OFF_MESHV], 4, 4, 0.0f, &m.meshv)) return refuse(why, "chain model lacks the mesh-vertex table");
  if (!optional_table(cmod, n, cmod[LM_H_NMESHN], cmod[LM_H_OFF_MESHN], 1, 1, -1.0f, &m.meshn)) return refuse(why, "chain model lacks the hull-vertex neighbour table");
  if (!optional_table(cmod, n, cmod[LM_H_NBPAIR], cmod[LM_H_OFF_BPT], LM_BP_SIZE, 1, 0.0f, &m.bpt)) return refuse(why, "chain model lacks the body-pair table");
  if (!optional_table(cmod, n, cmod[LM_H_NMESHADJ], cmod[LM_H_OFF_MESHADJ], 4, 64, 0.0f, &m.meshadj)) return refuse(why, "chain model lacks the hull adjacency blocks");      // (padded: a step of the hill climbing fetches eight entries at once)
  m.neq = (int)cmod[LM_H_NEQ]; m.off_eq = (int)cmod[LM_H_OFF_EQ];
  if (m.neq < 0 || (m.neq > 0 && (m.off_eq <= 0 || m.off_eq + m.neq * LM_EQ_SIZE > LM_CM_SIZE))) return refuse(why, "bad equality-record table");
  for (int i = 0; i < m.neq; i++) {
    const float* r = cm.data() + m.off_eq + i * LM_EQ_SIZE;
    const int lane = (int)r[LM_EQ_LANE], link = (int)r[LM_EQ_LINK];
    if (lane < 0 || lane >= LM_NCHAIN || link < 0 || link >= (int)cm[LM_CM_CHAINS + LM_C_NLINKS * LM_NCHAIN + lane]) return refuse(why, "equality record outside the chains");
  }
  return true;
}
}  // namespace lmp
