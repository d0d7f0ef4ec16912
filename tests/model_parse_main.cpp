// The host side of lm_model_create — loco_mujoco_amd/csrc/lm_model_parse.h and lm_families.h — without a device
// (tests/test_model_parse_host.py builds this with g++ -fsanitize=address,undefined and runs it as a child process: exit status 0 and
// no sanitizer report). Every blob lives in a heap buffer of exactly its size, so a read past its end is a sanitizer report.
//   model_parse parse FILE...   one line per chain-model blob (raw float64): the kernel family and the derived facts
//   model_parse cuts FILE...    the blob cut to the header, to header + constant table and one double short of the end of each optional
//                               table it has (muscle, geom-pair, mesh vertex, neighbour, body-pair, adjacency): each cut must be refused
//                               with a message, the whole blob must parse
//   model_parse pokes FILE...   the refusals that guard reads outside the buffer: a chain's geom count and link count at the largest value
//                               whose reads stay inside (must not be refused for it, and no sanitizer report) and one more (refused);
//                               an optional table's count / offset negative, not a number, huge, beyond the blob (refused)
//   model_parse instances FILE...   one line per blob: the family and the instantiation of its regular kernel — links and contact slots per chain,
//                               integrator, compiled-in cone (-1: read at run time), muscles per chain, pair pass (lm_families.h family(),
//                               generic_instance) — that the library launches for it; family -1: the refusal's reason
//   model_parse kinds           one line per family id: which of the LMK_* kinds the family table says it has
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../loco_mujoco_amd/csrc/lm_families.h"
#include "../loco_mujoco_amd/csrc/lm_model_parse.h"

namespace {

// the first n doubles of the file, in an allocation of exactly n doubles
std::unique_ptr<double[]> exact(const std::vector<double>& all, size_t n) {
  std::unique_ptr<double[]> p(new double[n]);
  memcpy(p.get(), all.data(), sizeof(double) * n);
  return p;
}

bool load(const char* path, std::vector<double>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(double);
  fseek(f, 0, SEEK_SET);
  out->resize(n);
  const bool ok = fread(out->data(), sizeof(double), n, f) == n;
  fclose(f);
  return ok;
}

std::string stem(const char* path) {
  std::string s = path;
  const size_t slash = s.rfind('/'), dot = s.rfind('.');
  return s.substr(slash == std::string::npos ? 0 : slash + 1, dot - (slash == std::string::npos ? 0 : slash + 1));
}

// what the two tables say together: family f has a kernel of kind k (the library's answer: lm_lds_bytes, from the objects themselves)
bool has_kind(const lmk::Family& f, int k) {
  const lmk::Kind& kd = lmk::kKinds[k];
  return f.present && (k == lmk::LMK_FWD || ((kd.layout == lmk::kPlain || f.specialised()) && (kd.DR == 0 || f.env_params())));
}

int family_of(const lmp::ParsedModel& m) {
  return lmk::pick_family({m.T.max_links, m.T.max_contacts, m.integrator, m.cone, m.T.na, m.T.npair, m.T.all_pyr3 != 0, m.root_xyz}, false);
}

int parse(const char* path) {
  std::vector<double> all;
  if (!load(path, &all)) { printf("%s: cannot read\n", path); return 1; }
  lmp::ParsedModel m;
  std::string why;
  if (!lmp::parse_model(exact(all, all.size()).get(), all.size(), &m, &why)) { printf("%s refused: %s\n", stem(path).c_str(), why.c_str()); return 1; }
  printf("%s family %d nv %d nu %d nobs %d max_links %d max_contacts %d npair %d na %d cm_used %d all_pyr3 %d root_xyz %d\n", stem(path).c_str(), family_of(m),
         m.T.nv, m.T.nu, m.T.nobs, m.T.max_links, m.T.max_contacts, m.T.npair, m.T.na, m.T.cm_used, m.T.all_pyr3, (int)m.root_xyz);
  // the tables as lm_model_create uploads them: today's padding
  const size_t ngp = (size_t)all[LM_H_NGPAIR], nmv = (size_t)all[LM_H_NMESHV], nmn = (size_t)all[LM_H_NMESHN], nbp = (size_t)all[LM_H_NBPAIR], nadj = (size_t)all[LM_H_NMESHADJ];
  const bool sizes = m.cm.size() == LM_CM_SIZE && m.gt.size() == LM_GT_SIZE && m.mt.size() == (m.T.na > 0 ? (size_t)LM_MT_SIZE : 0) && m.gpt.size() == ngp * LM_GPAIR_SIZE + 1 &&
                     m.n_gpt_floats == (int)(ngp * LM_GPAIR_SIZE) && m.meshv.size() == 4 * nmv + 4 && m.meshn.size() == nmn + 1 && m.meshn.back() == -1.0f &&
                     m.bpt.size() == nbp * LM_BP_SIZE + 1 && m.meshadj.size() == 4 * nadj + 64 && m.nominal.size() == (size_t)3 * m.T.nv;
  if (!sizes) { printf("%s: table sizes\n", stem(path).c_str()); return 1; }
  return 0;
}

int instance(const char* path) {
  std::vector<double> all;
  if (!load(path, &all)) { printf("%s: cannot read\n", path); return 1; }
  lmp::ParsedModel m;
  std::string why;
  if (!lmp::parse_model(exact(all, all.size()).get(), all.size(), &m, &why)) { printf("%s refused: %s\n", stem(path).c_str(), why.c_str()); return 1; }
  const int id = family_of(m);
  if (id < 0) {
    printf("%s family -1 refused: %s\n", stem(path).c_str(), lmk::no_family_reason({m.T.max_links, m.T.max_contacts, m.integrator, m.cone, m.T.na, m.T.npair, m.T.all_pyr3 != 0, m.root_xyz}));
    return 0;
  }
  const lmk::Family f = id == LM_GENERIC_FAMILY ? lmk::generic_instance(m.T.max_links, m.integrator == LM_INT_RK4) : lmk::family(id);
  printf("%s family %d present %d MC %d NS %d RK4 %d CONE %d NM %d PM %d\n", stem(path).c_str(), id, (int)f.present, f.MC, f.NS, (int)f.RK4, f.CONE, f.NM, f.PM);
  return 0;
}

int cuts(const char* path) {
  std::vector<double> all;
  if (!load(path, &all)) { printf("%s: cannot read\n", path); return 1; }
  const size_t n = all.size();
  lmp::ParsedModel m;
  std::string why;
  if (!lmp::parse_model(exact(all, n).get(), n, &m, &why)) { printf("%s refused: %s\n", stem(path).c_str(), why.c_str()); return 1; }
  struct Cut { const char* what; size_t at; };
  std::vector<Cut> list = {{"header", LM_HEADER_SIZE}, {"header + constant table", LM_HEADER_SIZE + LM_CM_SIZE}};
  auto table = [&](const char* what, int count_slot, int off_slot, size_t rec) {
    const size_t cnt = (size_t)all[count_slot];
    if (cnt > 0) list.push_back({what, (size_t)all[off_slot] + cnt * rec - 1});
  };
  if (all[LM_H_NMUSCLE] > 0) list.push_back({"muscle table", (size_t)LM_HEADER_SIZE + LM_CM_SIZE + LM_GT_SIZE + LM_MT_SIZE - 1});
  table("geom-pair table", LM_H_NGPAIR, LM_H_OFF_GPT, LM_GPAIR_SIZE);
  table("mesh-vertex table", LM_H_NMESHV, LM_H_OFF_MESHV, 4);
  table("neighbour table", LM_H_NMESHN, LM_H_OFF_MESHN, 1);
  table("body-pair table", LM_H_NBPAIR, LM_H_OFF_BPT, LM_BP_SIZE);
  table("adjacency blocks", LM_H_NMESHADJ, LM_H_OFF_MESHADJ, 4);
  for (const Cut& c : list) {
    if (c.at >= n) { printf("%s: the %s ends outside the blob\n", stem(path).c_str(), c.what); return 1; }
    why.clear();
    const bool ok = lmp::parse_model(exact(all, c.at).get(), c.at, &m, &why);
    printf("%s cut at %zu of %zu (%s): %s\n", stem(path).c_str(), c.at, n, c.what, ok ? "ACCEPTED" : why.c_str());
    if (ok || why.empty()) return 1;
  }
  printf("%s: %zu cuts refused\n", stem(path).c_str(), list.size());
  return 0;
}

// the blob with slot `at` set to `v`: 0 parsed, 1 refused with `msg`, 2 refused with something else
int poked(const std::vector<double>& all, size_t at, double v, const char* msg, const char* what) {
  std::vector<double> b = all;
  b[at] = v;
  lmp::ParsedModel m;
  std::string why;
  const bool ok = lmp::parse_model(exact(b, b.size()).get(), b.size(), &m, &why);
  printf("  slot %zu = %g (%s): %s\n", at, v, what, ok ? "parsed" : why.c_str());
  return ok ? 0 : (why == msg ? 1 : 2);
}

int pokes(const char* path) {
  std::vector<double> all;
  if (!load(path, &all)) { printf("%s: cannot read\n", path); return 1; }
  const size_t n = all.size();
  printf("%s pokes\n", stem(path).c_str());
  int bad = 0;
  const char* geoms = "a chain's geom count runs past the chain model";
  const char* links = "a chain's link count runs past the constant table";
  for (int c = 0; c < LM_NCHAIN; c += 3) {
    // the largest geom count of chain c whose last condim slot lies inside the blob, and the largest link count whose last dof index lies
    // inside the constant table (the furthest reads of the all_pyr3 loop and of the nominal table)
    size_t ng = 1, nl = 1;
    while (LM_HEADER_SIZE + LM_CM_SIZE + (ng * LM_G_SIZE + LM_G_DIM) * LM_NCHAIN + c < n) ng++;
    while (LM_CM_CHAINS + (LM_C_LINKS + nl * LM_LINK_SIZE + LM_D_DOF) * LM_NCHAIN + c < (size_t)LM_CM_SIZE) nl++;
    const size_t ng_at = LM_HEADER_SIZE + LM_CM_CHAINS + LM_C_NGEOMS * LM_NCHAIN + c, nl_at = LM_HEADER_SIZE + LM_CM_CHAINS + LM_C_NLINKS * LM_NCHAIN + c;
    if (all[LM_H_CONE] == LM_CONE_PYRAMIDAL) bad += poked(all, ng_at, (double)ng, geoms, "inside") == 1 || poked(all, ng_at, (double)ng + 1, geoms, "outside") != 1 || poked(all, ng_at, 1e9, geoms, "outside") != 1;
    bad += poked(all, nl_at, (double)nl, links, "inside") == 1 || poked(all, nl_at, (double)nl + 1, links, "outside") != 1 || poked(all, nl_at, 2e9, links, "outside") != 1;
  }
  if (all[LM_H_NGPAIR] > 0) {
    const char* lacks = "chain model lacks the geom-pair table";
    const double nan = std::nan(""), count_bad[] = {-5.0, nan, 1e300, (double)n + 1}, off_bad[] = {-5.0, nan, 1e300, (double)n + 1, (double)n - 1};
    for (double v : count_bad) bad += poked(all, LM_H_NGPAIR, v, lacks, "count") != 1;
    for (double v : off_bad) bad += poked(all, LM_H_OFF_GPT, v, lacks, "offset") != 1;
    bad += poked(all, LM_H_OFF_GPT, all[LM_H_OFF_GPT], lacks, "as it was") != 0;
  }
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  int bad = 0;
  if (mode == "kinds") {
    for (int f = -1; f <= lmk::LMK_NFAMILY; f++) {
      printf("family %d kinds", f);
      for (int k = 0; k < lmk::LMK_NKINDS; k++) printf(" %d", (int)has_kind(lmk::family(f), k));
      printf("\n");
    }
  } else {
    for (int i = 2; i < argc; i++) bad += mode == "cuts" ? cuts(argv[i]) : mode == "pokes" ? pokes(argv[i]) : mode == "instances" ? instance(argv[i]) : parse(argv[i]);
  }
  if (bad) return 1;
  printf("model parse: ok\n");
  return 0;
}
