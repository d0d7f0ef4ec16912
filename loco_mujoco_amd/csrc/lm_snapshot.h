// lm_snapshot.h — device-side snapshots of a batch (include/locohip.h lm_snapshot_*): the segment table, the index walk and the one
// copy kernel behind save, restore and fork. The per-environment state of a batch is a closed set of device arrays (lm_kernels.hip
// struct lm_batch); a snapshot is one device allocation that holds a copy of each, segment after segment.
//
//   SoA segments   [rows][N] elements of 1 or 4 bytes (qpos, qvel, warm, goal, act, slack, dofprm, ep_step, ep_count, premark, reward,
//                  done, flags, var, vdirty, vgen): environment e owns element e of every row
//   AoS segments   [N][row_bytes] (obs, mprc, vdraws, the model compiler's slots of vrec / vgt / vgpt): environment e owns row e
//
// Two walks over the table, both in plain C++ for host and device (tests/snapshot_walk_main.cpp runs them on the host under the
// address and undefined-behaviour sanitizers against a naive loop):
//   identity (save; restore of every environment's own state): a segment is one byte range, copied in units of 16 bytes of the
//                  DESTINATION: unit 0 of a segment is the head up to the destination's first 16-byte boundary, the last unit the
//                  tail; nothing is assumed about the alignment of either side (N = 37: rows start at multiples of 148 bytes)
//   gather  (restore with a source list: environment e takes the saved state of environment src[e]): SoA segments one element per
//                  unit, consecutive units = consecutive e of one row (coalesced stores, gathered loads snap[r][src[e]]); AoS segments
//                  one piece (16 bytes where row and bases allow, else 8 / 4 / 1) per unit, consecutive units = consecutive pieces
//                  of one row. An entry of src outside [0, N) yields no operation: no address is formed from it.
#ifndef LM_SNAPSHOT_H
#define LM_SNAPSHOT_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LMS_HD __host__ __device__
#else
#define LMS_HD
#endif

namespace lms {

constexpr int kMaxSeg = 24;
constexpr long long kSegAlign = 256;      // every segment starts at a multiple of this in the snapshot (hipMalloc's own alignment)
enum { kSoA = 0, kAoS = 1 };

struct Seg {
  unsigned char* ptr;      // the batch's array
  long long off;           // where its copy starts in the snapshot, bytes
  long long bytes;         // its size
  long long row_bytes;     // AoS: bytes of one environment's row (SoA: unused)
  long long id_first;      // first unit of this segment in the identity walk
  long long ga_first;      // ... and in the gather walk
  int rows;                // SoA: rows of N elements (AoS: unused)
  int elem;                // SoA: bytes per element; AoS: bytes per piece
  int kind;
  int pad_;
};

struct Table {
  int n, N;
  long long bytes;                 // of the whole snapshot
  long long id_units, ga_units;    // units of the two walks
  Seg seg[kMaxSeg];
};

struct Op {
  const unsigned char* src;
  unsigned char* dst;
  int n;                   // bytes to copy, 0: nothing
};

// ---- building the table (host)
inline void table_init(Table* t, int N) { memset(t, 0, sizeof(*t)); t->N = N; }

inline bool table_push(Table* t, void* ptr, int kind, int rows, int elem, long long row_bytes) {
  if (t->n >= kMaxSeg) return false;
  Seg& s = t->seg[t->n];
  s.ptr = static_cast<unsigned char*>(ptr); s.kind = kind; s.rows = rows; s.elem = elem; s.row_bytes = row_bytes;
  s.bytes = kind == kSoA ? (long long)rows * t->N * elem : row_bytes * t->N;
  s.off = (t->bytes + kSegAlign - 1) / kSegAlign * kSegAlign;
  s.id_first = t->id_units; s.ga_first = t->ga_units;
  t->id_units += 1 + (s.bytes + 15) / 16;                                  // the head unit + 16-byte units up to the tail
  t->ga_units += kind == kSoA ? (long long)rows * t->N : (row_bytes / elem) * t->N;
  t->bytes = s.off + s.bytes;
  t->n++;
  return true;
}
inline bool table_add_soa(Table* t, void* ptr, int rows, int elem) { return table_push(t, ptr, kSoA, rows, elem, 0); }
// the piece of an AoS segment: the widest of 16 / 8 / 4 / 1 bytes that divides the row and the array's address (the snapshot side starts
// at a multiple of kSegAlign of an allocation that is itself aligned to 16 bytes or better)
inline bool table_add_aos(Table* t, void* ptr, long long row_bytes) {
  int piece = 16;
  while (piece > 1 && (row_bytes % piece != 0 || reinterpret_cast<uintptr_t>(ptr) % piece != 0)) piece = piece == 16 ? 8 : (piece == 8 ? 4 : 1);
  return table_push(t, ptr, kAoS, 0, piece, row_bytes);
}

// ---- the walks (host and device)
LMS_HD inline int seg_of(const Table& t, long long u, bool gather) {
  int i = 0;
  while (i + 1 < t.n && u >= (gather ? t.seg[i + 1].ga_first : t.seg[i + 1].id_first)) i++;
  return i;
}

// unit u of the identity walk: restore = 0 copies batch -> snapshot, 1 snapshot -> batch
LMS_HD inline Op walk_identity(const Table& t, unsigned char* snap, int restore, long long u) {
  Op op = {nullptr, nullptr, 0};
  if (u < 0 || u >= t.id_units) return op;
  const Seg& s = t.seg[seg_of(t, u, false)];
  const long long c = u - s.id_first;
  unsigned char* in_snap = snap + s.off;
  const unsigned char* src = restore ? in_snap : s.ptr;
  unsigned char* dst = restore ? s.ptr : in_snap;
  long long head = (16 - (long long)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  if (head > s.bytes) head = s.bytes;
  const long long lo = c == 0 ? 0 : head + 16 * (c - 1);
  long long hi = c == 0 ? head : lo + 16;
  if (hi > s.bytes) hi = s.bytes;
  if (lo >= hi) return op;
  op.src = src + lo; op.dst = dst + lo; op.n = (int)(hi - lo);
  return op;
}

// unit u of the gather walk (snapshot -> batch): environment e takes what environment src[e] saved
LMS_HD inline Op walk_gather(const Table& t, unsigned char* snap, const int32_t* src, long long u) {
  Op op = {nullptr, nullptr, 0};
  if (u < 0 || u >= t.ga_units) return op;
  const Seg& s = t.seg[seg_of(t, u, true)];
  const long long c = u - s.ga_first, N = t.N;
  long long e, k;          // environment; row (SoA) or piece of the row (AoS)
  const long long inner = s.kind == kSoA ? N : s.row_bytes / s.elem;
  if (c < 0x7fffffffll) { const unsigned q = (unsigned)c / (unsigned)inner; k = q; e = (unsigned)c - q * (unsigned)inner; }
  else { k = c / inner; e = c - k * inner; }
  if (s.kind == kAoS) { const long long x = e; e = k; k = x; }          // (AoS: the quotient is the environment, the remainder the piece)
  const int32_t from = src[e];
  if (from < 0 || from >= t.N) return op;                              // "keeps what it has": nothing read, nothing written
  if (s.kind == kSoA) {
    op.src = snap + s.off + (k * N + from) * s.elem;
    op.dst = s.ptr + (k * N + e) * s.elem;
  } else {
    op.src = snap + s.off + from * s.row_bytes + k * s.elem;
    op.dst = s.ptr + e * s.row_bytes + k * s.elem;
  }
  op.n = s.elem;
  return op;
}

// one operation: 16 / 8 / 4 bytes in one access where both sides are aligned for it, bytes otherwise (heads, tails, byte arrays)
LMS_HD inline void copy_op(const Op& op) {
  if (op.n <= 0) return;
  const uintptr_t both = reinterpret_cast<uintptr_t>(op.src) | reinterpret_cast<uintptr_t>(op.dst);
  if (op.n == 16 && (both & 15) == 0) {
    struct alignas(16) V16 { uint32_t x, y, z, w; };
    *reinterpret_cast<V16*>(op.dst) = *reinterpret_cast<const V16*>(op.src);
  } else if (op.n == 8 && (both & 7) == 0) {
    struct alignas(8) V8 { uint32_t x, y; };
    *reinterpret_cast<V8*>(op.dst) = *reinterpret_cast<const V8*>(op.src);
  } else if ((op.n & 3) == 0 && (both & 3) == 0) {
    for (int i = 0; i < op.n; i += 4) *reinterpret_cast<uint32_t*>(op.dst + i) = *reinterpret_cast<const uint32_t*>(op.src + i);
  } else {
    for (int i = 0; i < op.n; i++) op.dst[i] = op.src[i];
  }
}

#if defined(__HIPCC__)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;       // grid-stride beyond that: 16 workgroups per compute unit keep the memory system busy

// THE kernel: one launch per save / restore over all segments. src == nullptr: the identity walk (restore = direction); otherwise the
// gather walk out of the snapshot. Consecutive lanes take consecutive units: 16 bytes each of one byte range, or consecutive
// environments of one SoA row, or consecutive pieces of one AoS row.
__global__ void __launch_bounds__(kThreads) snapshot_copy_kernel(const Table t, unsigned char* __restrict__ snap, const int32_t* __restrict__ src, int restore) {
  const long long total = src ? t.ga_units : t.id_units, stride = (long long)gridDim.x * kThreads;
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < total; u += stride)
    copy_op(src ? walk_gather(t, snap, src, u) : walk_identity(t, snap, restore, u));
}

inline void launch_copy(const Table& t, unsigned char* snap, const int32_t* d_src, int restore, hipStream_t stream) {
  const long long total = d_src ? t.ga_units : t.id_units;
  if (total <= 0) return;
  long long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(snapshot_copy_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, t, snap, d_src, restore);
}
#endif

}  // namespace lms
#endif
