// The per-unit work of loco_mujoco_amd/csrc/lm_state_io.h on the host (tests/test_state_io_host.py builds this with
// g++ -fsanitize=address,undefined and runs it as a child process: exit status 0 and no sanitizer report). Every array lives in a heap
// allocation of exactly its size, so an index outside it is a sanitizer report.
//   state_io_main walk                    gather, scatter under masks and restart for N = 37 and N = 1 against naive loops
//   state_io_main rows SEED GID COUNT ROWS ...   per quadruple one line: the reset-table row an environment with global id GID and
//                                         episode count COUNT (before the restart) draws from a table of ROWS rows under SEED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../loco_mujoco_amd/csrc/lm_state_io.h"

namespace {

template <class T> struct Exact {      // n elements in an allocation of exactly n elements
  std::unique_ptr<T[]> p; size_t n;
  explicit Exact(size_t n_) : p(new T[n_ ? n_ : 1]), n(n_) {}
  T* get() { return p.get(); }
  T& operator[](size_t i) { return p[i]; }
  bool same(const Exact& o) const { return n == o.n && memcmp(p.get(), o.p.get(), sizeof(T) * n) == 0; }
  void copy(const Exact& o) { memcpy(p.get(), o.p.get(), sizeof(T) * n); }
};

unsigned long long lcg = 12345;
float rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (float)((lcg >> 40) & 0xFFFF) / 65536.0f - 0.5f; }

// the arrays of one batch
struct Arrays {
  int N, nv, na, ngoal, nobs, ngrf, rows;
  Exact<float> qpos, qvel, warm, act, goal, slack, obs, dofprm, table, drspec;
  Exact<int> ep_step, premark, var, qobs, vobs;
  Exact<unsigned> ep_count;
  Exact<unsigned char> vdirty;
  Arrays(int N_, int nv_, int na_, int ngoal_, int ngrf_, int rows_)
      : N(N_), nv(nv_), na(na_), ngoal(ngoal_), nobs(2 * nv_ - 3 + ngoal_ + ngrf_), ngrf(ngrf_), rows(rows_), qpos((size_t)nv_ * N_), qvel((size_t)nv_ * N_),
        warm((size_t)nv_ * N_), act((size_t)na_ * N_), goal((size_t)4 * N_), slack((size_t)12 * N_), obs((size_t)N_ * nobs), dofprm((size_t)3 * nv_ * N_),
        table((size_t)rows_ * (2 * nv_ + ngoal_)), drspec((size_t)9 * nv_), ep_step(N_), premark(N_), var(N_), qobs(nv_), vobs(nv_), ep_count(N_), vdirty(N_) {
    // dofs 0 and 1 are not observed as positions, dof 2 not as a velocity: [q(2..) | v(all but 2) | goal | foot forces]
    int col = 0;
    for (int d = 0; d < nv; d++) qobs[d] = d < 2 ? -1 : col++;
    for (int d = 0; d < nv; d++) vobs[d] = d == 2 ? -1 : col++;
    for (size_t i = 0; i < qpos.n; i++) { qpos[i] = rnd(); qvel[i] = rnd(); warm[i] = rnd(); }
    for (size_t i = 0; i < act.n; i++) act[i] = rnd();
    for (size_t i = 0; i < goal.n; i++) goal[i] = rnd();
    for (size_t i = 0; i < slack.n; i++) slack[i] = rnd();
    for (size_t i = 0; i < obs.n; i++) obs[i] = -7.0f;
    for (size_t i = 0; i < dofprm.n; i++) dofprm[i] = 0.25f + rnd() * 0.1f;
    for (size_t i = 0; i < table.n; i++) table[i] = rnd();
    for (int i = 0; i < 3 * nv; i++) { drspec[3 * i] = (float)(i % 4); drspec[3 * i + 1] = (i % 2) ? 0.1f : 2.0f; drspec[3 * i + 2] = (i % 2) ? 1.0f : 0.05f; }
    for (int e = 0; e < N; e++) { ep_step[e] = 3 + e; premark[e] = e & 1; var[e] = 7; ep_count[e] = e == 0 ? 0xFFFFFFFFu : (unsigned)(5 * e); vdirty[e] = 0; }
  }
  lmio::State state() {
    return {N, nv, na, ngoal, nobs, ngrf, qpos.get(), qvel.get(), warm.get(), na ? act.get() : nullptr, goal.get(), slack.get(), ep_step.get(), ep_count.get(),
            premark.get(), qobs.get(), vobs.get()};
  }
  void copy(const Arrays& o) {
    qpos.copy(o.qpos); qvel.copy(o.qvel); warm.copy(o.warm); act.copy(o.act); goal.copy(o.goal); slack.copy(o.slack); obs.copy(o.obs); dofprm.copy(o.dofprm);
    ep_step.copy(o.ep_step); premark.copy(o.premark); var.copy(o.var); ep_count.copy(o.ep_count); vdirty.copy(o.vdirty);
  }
  bool same(const Arrays& o) const {
    return qpos.same(o.qpos) && qvel.same(o.qvel) && warm.same(o.warm) && act.same(o.act) && goal.same(o.goal) && slack.same(o.slack) && obs.same(o.obs) &&
           dofprm.same(o.dofprm) && ep_step.same(o.ep_step) && premark.same(o.premark) && var.same(o.var) && ep_count.same(o.ep_count) && vdirty.same(o.vdirty);
  }
};

// the observation row of (q, v, g) the naive way: a row built column by column
void naive_obs(const Arrays& a, float* o, const float* q, const float* v, const float* g) {
  for (int col = 0; col < a.nobs; col++) {
    for (int d = 0; d < a.nv; d++) { if (a.qobs.p[d] == col) o[col] = q[d]; if (a.vobs.p[d] == col) o[col] = v[d]; }
    if (col >= a.nobs - a.ngrf - a.ngoal && col < a.nobs - a.ngrf) o[col] = g[col - (a.nobs - a.ngrf - a.ngoal)];
    if (col >= a.nobs - a.ngrf) o[col] = 0.0f;
  }
}
void naive_clear(Arrays& a, int e, bool zero_act) {
  for (int d = 0; d < a.nv; d++) a.warm[(size_t)d * a.N + e] = 0.0f;
  if (zero_act) for (int i = 0; i < a.na; i++) a.act[(size_t)i * a.N + e] = 0.0f;
  for (int j = 0; j < 12; j++) a.slack[(size_t)j * a.N + e] = 0.0f;
  a.ep_step[e] = 0; a.premark[e] = 0;
}

unsigned long long naive_mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

int fail(const char* what, int N, int variant) { printf("FAILED: %s (N = %d, case %d)\n", what, N, variant); return 1; }

int check_gather(int N) {
  Arrays a(N, 7, 3, 2, 3, 5);
  for (int variant = 0; variant < 3; variant++) {
    Exact<float> q((size_t)N * a.nv), v((size_t)N * a.nv), ac((size_t)N * a.na), g((size_t)N * a.ngoal);
    Exact<int32_t> st(N); Exact<uint32_t> cn(N);
    for (size_t i = 0; i < q.n; i++) { q[i] = -7.0f; v[i] = -7.0f; }
    for (size_t i = 0; i < ac.n; i++) ac[i] = -7.0f;
    for (size_t i = 0; i < g.n; i++) g[i] = -7.0f;
    for (int e = 0; e < N; e++) { st[e] = -7; cn[e] = 77; }
    // case 0: every output; 1: qpos and the episode count only; 2: everything but those
    const bool first = variant != 2, rest = variant != 1;
    const lmio::GatherArgs ga = {a.state(), first ? q.get() : nullptr, rest ? v.get() : nullptr, rest ? ac.get() : nullptr, rest ? g.get() : nullptr,
                                 rest ? st.get() : nullptr, first ? cn.get() : nullptr};
    const long long total = lmio::gather_units(ga.s);
    if (total != (long long)N * (2 * a.nv + a.na + a.ngoal + 2)) return fail("gather units", N, variant);
    for (long long u = -2; u < total + 2; u++) lmio::gather_unit(ga, u);      // (units outside the walk: no operation)
    for (int e = 0; e < N; e++) {
      for (int d = 0; d < a.nv; d++) {
        if (q[(size_t)e * a.nv + d] != (first ? a.qpos[(size_t)d * N + e] : -7.0f)) return fail("gather qpos", N, variant);
        if (v[(size_t)e * a.nv + d] != (rest ? a.qvel[(size_t)d * N + e] : -7.0f)) return fail("gather qvel", N, variant);
      }
      for (int i = 0; i < a.na; i++) if (ac[(size_t)e * a.na + i] != (rest ? a.act[(size_t)i * N + e] : -7.0f)) return fail("gather act", N, variant);
      for (int i = 0; i < a.ngoal; i++) if (g[(size_t)e * a.ngoal + i] != (rest ? a.goal[(size_t)i * N + e] : -7.0f)) return fail("gather goal", N, variant);
      if (st[e] != (rest ? a.ep_step[e] : -7) || cn[e] != (first ? a.ep_count[e] : 77u)) return fail("gather counters", N, variant);
    }
  }
  return 0;
}

// masks: 0 none set, 1 all set, 2 NULL, 3 every third and the last
void make_mask(int N, int kind, Exact<uint8_t>& m) { for (int e = 0; e < N; e++) m[e] = kind == 0 ? 0 : kind == 1 ? 1 : (e % 3 == 1 || e == N - 1) ? 200 : 0; }

int check_scatter(int N) {
  for (int variant = 0; variant < 16; variant++) {
    const int mk = variant & 3; const bool with_act = variant & 4, with_goal = variant & 8;
    Arrays a(N, 7, variant == 5 ? 0 : 3, 2, 3, 5), want(N, 7, variant == 5 ? 0 : 3, 2, 3, 5);
    want.copy(a);
    Exact<float> q((size_t)N * a.nv), v((size_t)N * a.nv), ac((size_t)N * a.na), g((size_t)N * a.ngoal);
    for (size_t i = 0; i < q.n; i++) { q[i] = rnd(); v[i] = rnd(); }
    for (size_t i = 0; i < ac.n; i++) ac[i] = rnd();
    for (size_t i = 0; i < g.n; i++) g[i] = rnd();
    Exact<uint8_t> m(N);
    make_mask(N, mk, m);
    const lmio::ScatterArgs sa = {a.state(), q.get(), v.get(), with_act && a.na ? ac.get() : nullptr, with_goal ? g.get() : nullptr, mk == 2 ? nullptr : m.get(), a.obs.get()};
    for (int e = -1; e <= N; e++) lmio::scatter_env(sa, e);
    for (int e = 0; e < N; e++) {
      if (mk != 2 && !m[e]) continue;
      float gg[4];
      for (int d = 0; d < a.nv; d++) { want.qpos[(size_t)d * N + e] = q[(size_t)e * a.nv + d]; want.qvel[(size_t)d * N + e] = v[(size_t)e * a.nv + d]; }
      naive_clear(want, e, true);
      if (with_act) for (int i = 0; i < a.na; i++) want.act[(size_t)i * N + e] = ac[(size_t)e * a.na + i];
      for (int i = 0; i < a.ngoal; i++) { if (with_goal) want.goal[(size_t)i * N + e] = g[(size_t)e * a.ngoal + i]; gg[i] = want.goal[(size_t)i * N + e]; }
      naive_obs(want, want.obs.get() + (size_t)e * a.nobs, q.get() + (size_t)e * a.nv, v.get() + (size_t)e * a.nv, gg);
    }
    if (!a.same(want)) return fail("scatter", N, variant);
  }
  return 0;
}

int check_restart(int N) {
  for (int variant = 0; variant < 16; variant++) {
    const int mk = variant & 3, model = variant >> 2;      // model 0: nothing; 1: a pool of 3 with a draw of its own; 2: a pool of 5 following the rows; 3: the compiler's flag + redraw
    const int rows = 5;
    Arrays a(N, 7, 3, 2, 3, rows), want(N, 7, 3, 2, 3, rows);
    want.copy(a);
    Exact<uint8_t> m(N);
    make_mask(N, mk, m);
    const unsigned long long seed = 5; const long long off = 0x100000000ll + 1000;
    const int nvar = model == 1 ? 3 : model == 2 ? 5 : model == 3 ? N : 0, var_rows = model == 2 ? 1 : 0;
    const bool dr = model == 3 || model == 1;
    const lmio::RestartArgs ra = {a.state(), a.table.get(), rows, seed, off, model == 3 ? a.vdirty.get() : nullptr, a.var.get(), nvar, var_rows,
                                  dr ? a.dofprm.get() : nullptr, dr ? a.drspec.get() : nullptr, mk == 2 ? nullptr : m.get(), a.obs.get()};
    for (int e = -1; e <= N; e++) lmio::restart_env(ra, e);
    const int w = 2 * a.nv + a.ngoal;
    for (int e = 0; e < N; e++) {
      if (mk != 2 && !m[e]) continue;
      const unsigned ec = want.ep_count[e] + 1u;
      const unsigned long long gid = (unsigned long long)(off + e);
      const unsigned long long key = seed ^ naive_mix(gid * 2 + 1) ^ ((unsigned long long)ec << 32);
      const size_t r = (size_t)(naive_mix(key) % (unsigned long long)rows);
      const float* row = a.table.get() + r * w;
      for (int d = 0; d < a.nv; d++) { want.qpos[(size_t)d * N + e] = row[d]; want.qvel[(size_t)d * N + e] = row[a.nv + d]; }
      for (int i = 0; i < a.ngoal; i++) want.goal[(size_t)i * N + e] = row[2 * a.nv + i];
      naive_clear(want, e, true);
      want.ep_count[e] = ec;
      naive_obs(want, want.obs.get() + (size_t)e * a.nobs, row, row + a.nv, row + 2 * a.nv);
      if (model == 3) want.vdirty[e] = 1;
      if (model == 1) want.var[e] = (int)(naive_mix(key ^ 0xA24BAED4963EE407ull) % 3ull);
      if (model == 2) want.var[e] = (int)r;
      if (dr)
        for (int p = 0; p < 3; p++)
          for (int d = 0; d < a.nv; d++) {
            const float* sp = a.drspec.get() + ((size_t)p * a.nv + d) * 3;
            if ((int)sp[0] == 0) continue;
            const unsigned long long x = naive_mix(key ^ (unsigned long long)(d * 3 + p + 1) * 0xD6E8FEB86659FD93ull);
            const float u1 = ((float)(x >> 40) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)((x >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
            float val;
            if ((int)sp[0] == 2) val = sp[1] + (sp[2] - sp[1]) * u1;
            else val = fmaxf(fmaf(sp[2], sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2), sp[1]), 0.0f);
            want.dofprm[((size_t)p * a.nv + d) * N + e] = val;
          }
    }
    if (!a.same(want)) return fail("restart", N, variant);
    if (mk == 1 && model == 0 && N > 1) {      // not vacuous: the rows differ between environments, the first one's counter wrapped to 0
      bool differ = false;
      for (int e = 1; e < N; e++) differ = differ || a.qpos[e] != a.qpos[0];
      if (!differ || a.ep_count[0] != 0u) return fail("restart draws", N, variant);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "rows") == 0) {
    if ((argc - 2) % 4 != 0) return 2;
    for (int i = 2; i + 3 < argc; i += 4) {
      const unsigned long long seed = strtoull(argv[i], nullptr, 0);
      const long long gid = strtoll(argv[i + 1], nullptr, 0);
      const unsigned count = (unsigned)strtoull(argv[i + 2], nullptr, 0);
      const int rows = atoi(argv[i + 3]);
      printf("row %lld\n", lmio::restart_row(seed, gid, count + 1u, rows));
    }
    return 0;
  }
  int bad = 0;
  for (int N : {37, 1}) bad += check_gather(N) + check_scatter(N) + check_restart(N);
  if (bad) return 1;
  printf("state io: ok\n");
  return 0;
}
