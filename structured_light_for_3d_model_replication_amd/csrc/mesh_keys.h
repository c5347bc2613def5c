// mesh_keys.h -- what the mesh connectivity units share (included, never compiled alone):
// cloud_meshpost.hip (adjacency, smoothing, hole closing), cloud_decimate.hip
// (quadric edge collapse in rounds; §19) and cloud_audit.hip (edge classes, components; §22).  A
// directed pair (src, dst) is the 64-bit key src << 32 | dst; everything about connectivity is a
// radix sort of such keys, a flag pass, a scan and binary searches in the sorted keys.  The keys are 64-bit, another type than cloud_grid.hip's
// and cloud_mesh.hip's sorts, so rocPRIM is instantiated in each unit that includes this.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "cloud_grid.h"

namespace slgmeshpost {

using slgcloud::Bump;
using slgcloud::grid_of;

struct PostHdr {        // the mesh header's status, nV and nT where cloud_mesh.hip has them
  int32_t status;       // SLG_FILTER_BAD_INDEX: a triangle index outside 0 .. V - 1
  int32_t R;            // unused here
  int64_t nV, nT;       // adjacency: neighbour and boundary-neighbour entries; holes: nT = new triangles
  double unused[13];
  int64_t stats[8];     // holes: SLG_MESH_HOLES_STAT_*
};
static_assert(sizeof(PostHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(PostHdr, nV) == 8 && offsetof(PostHdr, nT) == 16 && offsetof(PostHdr, stats) == 128, "mesh.py's offsets");

__host__ __device__ inline uint64_t edge_key(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | (uint64_t)b; }
__device__ inline uint32_t key_src(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ inline uint32_t key_dst(uint64_t k) { return (uint32_t)(k & 0xFFFFFFFFull); }
// The first index whose key is >= k (n when none).
__device__ inline int64_t lower_bound(const uint64_t* __restrict__ s, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (s[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- sorts and scans
struct U8ToU64 {
  __host__ __device__ uint64_t operator()(uint8_t v) const { return v; }
};
// rocPRIM's scratch by a closed bound: 64-bit keys need 8 n + lookback; the scans (lookback states
// only, n / 4 + 1 MiB) run in the same region
static inline size_t sort_temp(size_t n) { return 12 * n + (4u << 20); }
static inline int fits(const char* who, hipError_t e, size_t need, size_t bound) {
  if (e != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM size query failed", who);
  if (need > bound)
    return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM asks for %lld bytes of scratch, the bound is %lld", who,
                             (long long)need, (long long)bound);
  return SLG_OK;
}
static inline int scan_u8(const char* who, const uint8_t* in, uint64_t* out, size_t n, void* temp, size_t tb, hipStream_t st) {
  auto it = rocprim::make_transform_iterator(in, U8ToU64());
  size_t need = 0;
  const hipError_t e = rocprim::exclusive_scan(nullptr, need, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
  if (int rc = fits(who, e, need, tb)) return rc;
  if (rocprim::exclusive_scan(temp, tb, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: scan failed", who);
  return SLG_OK;
}
// Keys hold a source of at most V (the sentinel) in their high half: 32 + bit length of V bits.
static inline int sort_keys(const char* who, const uint64_t* in, uint64_t* out, size_t n, int64_t V, void* temp, size_t tb,
                            hipStream_t st) {
  unsigned bits = 32;
  while (bits < 64 && ((uint64_t)V >> (bits - 32))) ++bits;
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_keys(nullptr, need, in, out, n, 0u, bits, st);
  if (int rc = fits(who, e, need, tb)) return rc;
  if (rocprim::radix_sort_keys(temp, tb, in, out, n, 0u, bits, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: radix sort failed", who);
  return SLG_OK;
}
// The same sort carrying a 32-bit value per key (cloud_audit.hip: an edge's position and direction
// bit).  A radix sort is stable: equal keys keep their values in input order.  rocPRIM's scratch by
// a closed bound: a second copy of the keys and of the values (12 n) and the lookback states.
static inline size_t sort_pairs_temp(size_t n) { return 16 * n + (4u << 20); }
static inline int sort_pairs(const char* who, const uint64_t* in, uint64_t* out, const uint32_t* vin, uint32_t* vout, size_t n,
                             int64_t V, void* temp, size_t tb, hipStream_t st) {
  unsigned bits = 32;
  while (bits < 64 && ((uint64_t)V >> (bits - 32))) ++bits;
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, in, out, vin, vout, n, 0u, bits, st);
  if (int rc = fits(who, e, need, tb)) return rc;
  if (rocprim::radix_sort_pairs(temp, tb, in, out, vin, vout, n, 0u, bits, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: radix sort failed", who);
  return SLG_OK;
}
// The workspace binding every entry point starts with; `sizer` is the function the text names.
static inline int bind(const char* who, const char* sizer, void* ws, int64_t ws_bytes, size_t need) {
  if (!ws || ((uintptr_t)ws & 255)) return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace NULL or not 256-byte aligned", who);
  if (ws_bytes < 0 || (size_t)ws_bytes < need)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace of %lld bytes, %s gives %lld", who, (long long)ws_bytes, sizer,
                             (long long)need);
  return SLG_OK;
}
// 3 T winding pairs in 32-bit positions, vertex ids in the key's halves
static inline bool counts_ok(int64_t nv, int64_t nt) { return nv > 0 && nt > 0 && nv < (1ll << 31) && nt <= (1ll << 30) / 3; }

namespace {

// ---------------------------------------------------------------- directed pairs
// Per triangle (a, b, c): the winding pairs a->b, b->c, c->a into k3 and, when k6 is given, the six
// pairs a->b, b->a, b->c, c->b, c->a, a->c.  An index outside 0 .. V - 1 sets the status word and
// turns the triangle's keys into the sentinel (V, 0), which sorts behind every pair.
__global__ __launch_bounds__(256)
void pair_keys_kernel(PostHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, int64_t nv, uint64_t* __restrict__ k3,
                      uint64_t* __restrict__ k6) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
  const bool bad = a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv;
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
  const uint64_t none = edge_key((uint32_t)nv, 0u);
  const uint32_t A = (uint32_t)a, Bv = (uint32_t)b, C = (uint32_t)c;
  k3[3 * t] = bad ? none : edge_key(A, Bv);
  k3[3 * t + 1] = bad ? none : edge_key(Bv, C);
  k3[3 * t + 2] = bad ? none : edge_key(C, A);
  if (!k6) return;
  k6[6 * t] = bad ? none : edge_key(A, Bv);
  k6[6 * t + 1] = bad ? none : edge_key(Bv, A);
  k6[6 * t + 2] = bad ? none : edge_key(Bv, C);
  k6[6 * t + 3] = bad ? none : edge_key(C, Bv);
  k6[6 * t + 4] = bad ? none : edge_key(C, A);
  k6[6 * t + 5] = bad ? none : edge_key(A, C);
}

// A CSR entry: the first of its equal keys, no self-pair, no sentinel.
__global__ __launch_bounds__(256)
void unique_flag_kernel(const uint64_t* __restrict__ s, int64_t n, int64_t nv, uint8_t* __restrict__ f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = s[i];
  f[i] = (key_src(k) < (uint64_t)nv && key_src(k) != key_dst(k) && (i == 0 || s[i - 1] != k)) ? 1 : 0;
}

// The winding pair (a, b) is a boundary edge iff (b, a) is not among the winding pairs.
__device__ inline bool boundary_rule(const uint64_t* __restrict__ d3, int64_t n, int64_t nv, int64_t i) {
  const uint64_t k = d3[i];
  if (key_src(k) >= (uint64_t)nv || (i > 0 && d3[i - 1] == k)) return false;
  const uint64_t rev = edge_key(key_dst(k), key_src(k));
  const int64_t lb = lower_bound(d3, n, rev);
  return !(lb < n && d3[lb] == rev);
}

__global__ __launch_bounds__(256)
void csr_neighbours_kernel(const PostHdr* hdr, const uint64_t* __restrict__ s, const uint8_t* __restrict__ f,
                           const uint64_t* __restrict__ pos, int64_t n, int32_t* __restrict__ out, int64_t n_out) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !f[i]) return;
  const uint64_t o = pos[i];
  if (o < (uint64_t)n_out) out[o] = (int32_t)key_dst(s[i]);
}

}  // namespace
}  // namespace slgmeshpost
