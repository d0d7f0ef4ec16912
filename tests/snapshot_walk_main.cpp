// The index walks of loco_mujoco_amd/csrc/lm_snapshot.h on the host, against a naive loop (tests/test_snapshot_host.py builds this
// with g++ -fsanitize=address,undefined and runs it as a child process: exit status 0 and no sanitizer report).
// Segment tables for N = 1, 37, 64 with SoA rows of 4-byte and 1-byte elements and AoS rows of 112 and 128 bytes (and one of 24 bytes:
// 8-byte pieces); the arrays are allocated with exactly their size, so a byte read or written outside one is a sanitizer report, and
// at odd offsets of their allocations, so that heads and tails of the 16-byte units occur. Save, identity restore, gathered restore
// with repeats, -1, N and INT_MIN in the source list.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../loco_mujoco_amd/csrc/lm_snapshot.h"

namespace {

struct Array { int kind, rows, elem; long long row_bytes; int skew; };      // skew: bytes the array starts behind a 16-byte boundary

const Array kArrays[] = {
    {lms::kSoA, 18, 4, 0, 0},  {lms::kSoA, 3, 4, 0, 4}, {lms::kSoA, 1, 1, 0, 0},   {lms::kSoA, 2, 1, 0, 3}, {lms::kAoS, 0, 0, 112, 0},
    {lms::kAoS, 0, 0, 128, 0}, {lms::kSoA, 1, 4, 0, 8}, {lms::kAoS, 0, 0, 24, 8},  {lms::kAoS, 0, 0, 148, 0}, {lms::kSoA, 12, 4, 0, 12},
};
constexpr int kNArrays = sizeof(kArrays) / sizeof(kArrays[0]);

struct Batch {
  int N;
  std::vector<unsigned char*> raw, ptr;
  std::vector<long long> bytes;
  lms::Table t;
  explicit Batch(int n) : N(n) {
    lms::table_init(&t, N);
    for (const Array& a : kArrays) {
      const long long b = a.kind == lms::kSoA ? (long long)a.rows * N * a.elem : a.row_bytes * N;
      unsigned char* r = static_cast<unsigned char*>(malloc((size_t)(b + a.skew)));      // 16-byte aligned, and tight: the sanitizer's redzone starts at the array's end
      raw.push_back(r); ptr.push_back(r + a.skew); bytes.push_back(b);
      const bool ok = a.kind == lms::kSoA ? lms::table_add_soa(&t, r + a.skew, a.rows, a.elem) : lms::table_add_aos(&t, r + a.skew, a.row_bytes);
      if (!ok) { fprintf(stderr, "segment table full\n"); exit(2); }
    }
  }
  ~Batch() { for (unsigned char* r : raw) free(r); }
  void fill(unsigned seed) {
    for (int i = 0; i < kNArrays; i++)
      for (long long k = 0; k < bytes[i]; k++) { seed = seed * 1664525u + 1013904223u; ptr[i][k] = (unsigned char)(seed >> 24); }
  }
  std::vector<std::vector<unsigned char>> copy() const {
    std::vector<std::vector<unsigned char>> c;
    for (int i = 0; i < kNArrays; i++) c.emplace_back(ptr[i], ptr[i] + bytes[i]);
    return c;
  }
};

int g_bad = 0;
void expect(bool ok, const char* what, int N, int i) {
  if (!ok) { g_bad++; fprintf(stderr, "N = %d, array %d: %s\n", N, i, what); }
}

// the bytes environment e owns in array i, in order
std::vector<unsigned char> env_bytes(const std::vector<unsigned char>& arr, const Array& a, int N, int e) {
  std::vector<unsigned char> out;
  if (a.kind == lms::kSoA) {
    for (int r = 0; r < a.rows; r++)
      for (int k = 0; k < a.elem; k++) out.push_back(arr[((size_t)r * N + e) * a.elem + k]);
  } else {
    for (long long k = 0; k < a.row_bytes; k++) out.push_back(arr[(size_t)e * a.row_bytes + k]);
  }
  return out;
}

void run(int N) {
  Batch b(N);
  const lms::Table& t = b.t;
  // the snapshot with a guard band on either side: the walks must not touch it
  const long long guard = 64;
  unsigned char* store = static_cast<unsigned char*>(aligned_alloc(256, (size_t)((t.bytes + 2 * guard + 255) / 256 * 256 + 256)));
  unsigned char* snap = store + 256;       // (256-byte aligned like a device allocation; `guard` bytes in front and behind are watched)
  memset(store, 0xA5, (size_t)((t.bytes + 2 * guard + 255) / 256 * 256 + 256));
  for (int i = 0; i < t.n; i++) expect(t.seg[i].off % lms::kSegAlign == 0 && t.seg[i].off + t.seg[i].bytes <= t.bytes, "segment outside the snapshot", N, i);
  for (int i = 0; i + 1 < t.n; i++) expect(t.seg[i].off + t.seg[i].bytes <= t.seg[i + 1].off, "segments overlap", N, i);
  expect(t.seg[4].elem == 16 && t.seg[5].elem == 16 && t.seg[7].elem == 8 && t.seg[8].elem == 4, "piece width", N, 4);

  // save
  b.fill(17u + N);
  const auto saved = b.copy();
  for (long long u = -1; u <= t.id_units; u++) lms::copy_op(lms::walk_identity(t, snap, 0, u));      // (-1 and id_units: no operation)
  for (int i = 0; i < kNArrays; i++) expect(memcmp(snap + t.seg[i].off, saved[i].data(), (size_t)b.bytes[i]) == 0, "save", N, i);
  for (long long k = 0; k < guard; k++) expect(snap[-1 - k] == 0xA5 && snap[t.bytes + k] == 0xA5, "save wrote outside the snapshot", N, -1);
  { const auto now = b.copy(); for (int i = 0; i < kNArrays; i++) expect(now[i] == saved[i], "save changed the batch", N, i); }

  // identity restore
  b.fill(99u + N);
  for (long long u = 0; u < t.id_units; u++) lms::copy_op(lms::walk_identity(t, snap, 1, u));
  { const auto now = b.copy(); for (int i = 0; i < kNArrays; i++) expect(now[i] == saved[i], "identity restore", N, i); }

  // gathered restore: repeats, "keep" entries of every kind
  b.fill(5u + N);
  const auto before = b.copy();
  std::vector<int32_t> src(N);
  for (int e = 0; e < N; e++) src[e] = (e * 7 + 3) % N;
  const int32_t keep[4] = {-1, N, INT_MIN, INT_MAX};
  for (int e = 1, k = 0; e < N; e += 5, k++) src[e] = keep[k % 4];
  for (int e = 2; e < N; e += 6) src[e] = N > 5 ? 5 : 0;                   // several environments take one source
  if (N == 1) src[0] = 0;
  for (long long u = -1; u <= t.ga_units; u++) lms::copy_op(lms::walk_gather(t, snap, src.data(), u));
  const auto now = b.copy();
  for (int i = 0; i < kNArrays; i++)
    for (int e = 0; e < N; e++) {
      const bool kept = src[e] < 0 || src[e] >= N;
      const auto want = kept ? env_bytes(before[i], kArrays[i], N, e) : env_bytes(saved[i], kArrays[i], N, src[e]);
      expect(env_bytes(now[i], kArrays[i], N, e) == want, kept ? "gather touched an environment that keeps its state" : "gather", N, i);
    }
  // the same with every entry out of range: nothing moves, and no address is formed (ubsan: pointer overflow; asan: the access)
  for (int e = 0; e < N; e++) src[e] = keep[e % 4];
  for (long long u = 0; u < t.ga_units; u++) {
    const lms::Op op = lms::walk_gather(t, snap, src.data(), u);
    expect(op.n == 0 && op.src == nullptr && op.dst == nullptr, "an out-of-range source formed an operation", N, -1);
  }
  for (long long k = 0; k < guard; k++) expect(snap[-1 - k] == 0xA5 && snap[t.bytes + k] == 0xA5, "restore wrote outside the snapshot", N, -1);
  free(store);
}

}  // namespace

int main() {
  for (int N : {1, 37, 64}) run(N);
  if (g_bad) { fprintf(stderr, "%d mismatches\n", g_bad); return 1; }
  printf("snapshot walks: ok\n");
  return 0;
}
