// The dof -> observation-column maps that loco_mujoco_amd/csrc/lm_model_parse.h derives from a chain-model blob (ParsedModel::qobs / vobs,
// read by lm_state_io.h), without a device (tests/test_state_io_host.py builds this with g++ -fsanitize=address,undefined and runs it as a
// child process). The blob lives in a heap buffer of exactly its size.
//   obs_maps_main FILE...   per blob (raw float64) two lines: "<name> qobs c0 c1 ..." and "<name> vobs c0 c1 ...", one column per dof
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../loco_mujoco_amd/csrc/lm_families.h"
#include "../loco_mujoco_amd/csrc/lm_model_parse.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { printf("%s: cannot read\n", argv[i]); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(double);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<double[]> blob(new double[n ? n : 1]);
    const bool ok = fread(blob.get(), sizeof(double), n, f) == n;
    fclose(f);
    if (!ok) { printf("%s: cannot read\n", argv[i]); return 1; }
    std::string name = argv[i];
    const size_t slash = name.rfind('/');
    if (slash != std::string::npos) name = name.substr(slash + 1);
    name = name.substr(0, name.rfind('.'));
    lmp::ParsedModel m;
    std::string why;
    if (!lmp::parse_model(blob.get(), n, &m, &why)) { printf("%s refused: %s\n", name.c_str(), why.c_str()); return 1; }
    if (m.qobs.size() != (size_t)m.T.nv || m.vobs.size() != (size_t)m.T.nv) { printf("%s: map sizes\n", name.c_str()); return 1; }
    printf("%s qobs", name.c_str());
    for (int c : m.qobs) printf(" %d", c);
    printf("\n%s vobs", name.c_str());
    for (int c : m.vobs) printf(" %d", c);
    printf("\n");
  }
  printf("obs maps: ok\n");
  return 0;
}
