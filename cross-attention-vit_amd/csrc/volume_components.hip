// Connected foreground components (include/xvit.h, "Connected foreground components"): every foreground voxel's label is the smallest flat
// index of its 6- or 26-connected component, the per-volume component table, and foreground boxes over the kept components only, which
// volume_bbox.hip's finish kernel turns into the sample crop and folds.  Block-based union-find (Komura; Playne & Hawick; Allegretti et
// al. in kind) in a fixed number of launches, with no host read-back and no host loop:
//
//   (0) zero    the accumulators and the size table of the workspace (nothing is pre-set: a graph replay is self-contained)
//   (1) tile    an 8 x 8 x 32 tile is labelled in LDS and written out: a voxel's label is the flat index of its tile-local root
//   (2) merge   voxels on a tile face unite with their neighbours in other tiles, in global memory
//   (3) flatten every voxel descends to its root
//   (4) count   size[root] += 1 per voxel, aggregated per wave and per workgroup first
//   (5) pick    the roots of a volume contend for the largest; the components and voxels at or above min_voxels are counted
//   (6) table   one thread per volume writes its record of comps
//   (7) boxes   partial boxes over the kept voxels, in the layout of volume_bbox.hip's, then that file's finish kernel
//
// Union-find on this machine.  L is the label array; a background voxel holds -1 from (1) on and never changes.
//   Invariants: every value ever stored in L[i] is <= i and lies in i's component, and a word only ever decreases.  In (2) and (3), where
//   two workgroups can touch one word, every write is a device-scope atomicMin; there is no path compression by plain stores.
//   Stale reads: the per-XCD L2s are not coherent for plain loads, so a load in (2) or (3) may return an older value of a word that another
//   workgroup has lowered.  By the invariants an older value is a larger ancestor in the same component, and whoever replaced it took on
//   the union of the old and the new value (below), so it still leads to the component's root at the end of the launch.  No loop's exit
//   depends on seeing another workgroup's store: there is no spinning, no flag and no ticket.
//   Termination: find(a) replaces a by L[a] < a until L[a] == a: it descends strictly, at most a steps.  unite(a, b) takes a = find(a),
//   b = find(b), leaves when a == b, orders them a > b and calls old = atomicMin(&L[a], b).  old == a: a was a root and now points to b,
//   done.  Otherwise old < a: L[a] holds min(old, b), and old and b remain to be united; it continues with (old, b).  The sum a + b falls
//   by at least one per round, so there are fewer than 2 nvox rounds.
//   Step caps: every such loop also counts its steps against a cap that correct code cannot reach (the tile size or nvox for a descent,
//   twice that for a union).  A lane that reaches it sets a bit of the volume's status word and leaves; a defect shows as status != 0 in
//   comps, never as a hung card.
//   Sizes: exact integers.  One atomic add per voxel into size[root] would serialise a 3 M-voxel component on one word, so (4) first
//   takes the smallest root of the workgroup's 4096 voxels as its dominant root and counts that in registers and LDS (one global add per
//   workgroup); the other roots of a wave are matched lane against lane with ballots and added once per (wave, slot, root).
// The smallest index of a component, its size and the kept set do not depend on the execution order: every output is bit-reproducible.
#include <math.h>

#include "volume_box.h"

namespace xvit {

constexpr int kCcTZ = 8, kCcTY = 8, kCcTX = 32;   // the tile; a row of a tile is one 32-bit mask
constexpr int kCcRows = kCcTZ * kCcTY, kCcTile = kCcRows * kCcTX;
constexpr int kCcThreads = 256;
constexpr int kCcPerThread = kCcTile / kCcThreads;
constexpr int kCcCountChunk = 16 * kCcThreads;    // voxels per workgroup of (4)
constexpr int kCcBadTile = 1, kCcBadMerge = 2, kCcBadFlatten = 4;   // bits of the status word

// per-volume accumulators at the head of the workspace: 8 ints
struct CcAcc {
  unsigned long long best;   // (size << 32) | (0x7fffffff - root) of the largest component; 0: none
  int ncomp, nkept, kept_vox, status, pad[2];   // nkept, kept_vox: components / voxels at or above min_voxels
};
static_assert(sizeof(CcAcc) == 32, "CcAcc is 8 ints");

struct CcGeom {
  int Ds, Hs, Ws, tz, ty, tx;   // sizes and tiles per axis
  int64_t nvox;
};

static int64_t cc_acc_bytes(int nvol) { return (int64_t)nvol * (int64_t)sizeof(CcAcc); }
static int64_t cc_size_bytes(int nvol, int64_t nvox) { return ((int64_t)nvol * nvox * 4 + 15) & ~(int64_t)15; }

// ------------------------------------------------------------------------------------------
// (0) zero
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcThreads) cc_zero_kernel(int4* __restrict__ p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kCcThreads) p[i] = int4{0, 0, 0, 0};
}

// ------------------------------------------------------------------------------------------
// (1) tile.  Labels in LDS are tile-local indices (lz * 8 + ly) * 32 + lx, which order the tile's voxels as their flat indices do.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(const int* lab, int a, int& bad) {
  for (int step = 0; step <= kCcTile; ++step) {
    const int p = lab[a];
    if (p == a) return a;
    a = p;
  }
  bad = 1;
  return a;
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b, int& bad) {
  for (int step = 0; step <= 2 * kCcTile; ++step) {
    a = lds_find(lab, a, bad), b = lds_find(lab, b, bad);
    if (a == b || bad) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
  bad = 1;
}

// voxel (row, x) of the tile against the row `nrow` of the same tile: unite with what it touches there
template <int CONN>
__device__ __forceinline__ void tile_unite_row(int* lab, const uint32_t* rowmask, int row, int x, uint32_t m, int nrow, int& bad) {
  const uint32_t nm = rowmask[nrow];
  const int i = row * kCcTX + x, n = nrow * kCcTX + x;
  const bool left = x > 0 && ((m >> (x - 1)) & 1u);   // the voxel before this one is foreground: the same run, already one set
  if ((nm >> x) & 1u) {
    // the voxel before this one touches the same run of the other row through its own column: it does the union
    if (!(left && ((nm >> (x - 1)) & 1u))) lds_unite(lab, i, n, bad);
    return;
  }
  if (CONN == 26) {   // column x of the other row is background: x - 1 and x + 1 there belong to two different runs
    if (x > 0 && ((nm >> (x - 1)) & 1u)) lds_unite(lab, i, n - 1, bad);
    if (x < kCcTX - 1 && ((nm >> (x + 1)) & 1u)) lds_unite(lab, i, n + 1, bad);
  }
}

template <class S, int CONN>
__global__ void __launch_bounds__(kCcThreads) cc_tile_kernel(const S* __restrict__ src, int* __restrict__ labels, CcAcc* __restrict__ acc, CcGeom g, float fg) {
  constexpr int E = 16 / (int)sizeof(S), SEGS = kCcTX / E;   // voxels per 16-byte run, runs per tile row
  __shared__ uint32_t rowmask[kCcRows];
  __shared__ int lab[kCcTile];
  const int tid = threadIdx.x;
  const int per_vol = g.tz * g.ty * g.tx;
  const int vol = blockIdx.x / per_vol;
  int t = blockIdx.x - vol * per_vol;
  const int bx = t % g.tx;
  t /= g.tx;
  const int by = t % g.ty, bz = t / g.ty;
  const int z0 = bz * kCcTZ, y0 = by * kCcTY, x0 = bx * kCcTX;
  const S* __restrict__ vsrc = src + (int64_t)vol * g.nvox;
  int* __restrict__ vlab = labels + (int64_t)vol * g.nvox;

  if (tid < kCcRows) rowmask[tid] = 0;
  __syncthreads();
  // the foreground masks: 16-byte loads where the run lies inside the row and is aligned (rows are not aligned, and a volume's base is
  // only element-aligned when nvox is odd), element by element otherwise
  for (int sidx = tid; sidx < kCcRows * SEGS; sidx += kCcThreads) {
    const int row = sidx / SEGS, sg = sidx - row * SEGS;
    const int z = z0 + (row >> 3), y = y0 + (row & 7), x = x0 + sg * E;
    if (z >= g.Ds || y >= g.Hs || x >= g.Ws) continue;
    const S* p = vsrc + ((int64_t)z * g.Hs + y) * g.Ws + x;
    uint32_t m = 0;
    if (x + E <= g.Ws && ((uintptr_t)p & 15) == 0) {
      m = fg_mask<S>(*(const uint4*)p, fg);
    } else {
      for (int e = 0; e < E && x + e < g.Ws; ++e) m |= (uint32_t)(src_f(p[e]) > fg) << e;
    }
    if (m) atomicOr(&rowmask[row], m << (sg * E));
  }
  __syncthreads();
  // a voxel starts at the first voxel of its run along x: the unions along x are done
#pragma unroll
  for (int k = 0; k < kCcPerThread; ++k) {
    const int i = tid + k * kCcThreads, row = i >> 5, x = i & 31;
    const uint32_t m = rowmask[row];
    const uint32_t gaps = ~m & ((1u << x) - 1u);   // background before x
    lab[i] = ((m >> x) & 1u) ? row * kCcTX + (gaps ? 32 - __clz(gaps) : 0) : -1;
  }
  __syncthreads();
  int bad = 0;
#pragma unroll
  for (int k = 0; k < kCcPerThread; ++k) {
    const int i = tid + k * kCcThreads, row = i >> 5, x = i & 31;
    const uint32_t m = rowmask[row];
    if (!((m >> x) & 1u)) continue;
    const int lz = row >> 3, ly = row & 7;
    if (ly > 0) tile_unite_row<CONN>(lab, rowmask, row, x, m, row - 1, bad);
    if (lz > 0) tile_unite_row<CONN>(lab, rowmask, row, x, m, row - kCcTY, bad);
    if (CONN == 26 && lz > 0) {
      if (ly > 0) tile_unite_row<CONN>(lab, rowmask, row, x, m, row - kCcTY - 1, bad);
      if (ly < kCcTY - 1) tile_unite_row<CONN>(lab, rowmask, row, x, m, row - kCcTY + 1, bad);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kCcPerThread; ++k) {
    const int i = tid + k * kCcThreads, row = i >> 5, x = i & 31;
    const int z = z0 + (row >> 3), y = y0 + (row & 7);
    if (z >= g.Ds || y >= g.Hs || x0 + x >= g.Ws) continue;
    int out = -1;
    if (lab[i] >= 0) {
      const int r = lds_find(lab, i, bad);
      out = (int)(((int64_t)(z0 + (r >> 8)) * g.Hs + (y0 + ((r >> 5) & 7))) * g.Ws + x0 + (r & 31));
    }
    vlab[((int64_t)z * g.Hs + y) * g.Ws + x0 + x] = out;
  }
  if (bad) atomicOr(&acc[vol].status, kCcBadTile);
}

// ------------------------------------------------------------------------------------------
// (2) merge and (3) flatten, in global memory.  Loads of L are relaxed device-scope atomic loads, so that no value is kept in a register
// or served by this CU's L1 across an atomicMin; the argument above does not need them to be fresh.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(const int* L, int a, uint32_t cap, int& bad) {
  for (uint32_t step = 0; step <= cap; ++step) {
    const int p = g_load(L + a);
    if (p == a) return a;
    a = p;
  }
  bad = 1;
  return a;
}
__device__ __forceinline__ void g_unite(int* L, int a, int b, uint32_t cap, int& bad) {
  for (uint32_t step = 0; step <= 2 * cap; ++step) {   // cap = nvox < 2^31
    a = g_find(L, a, cap, bad), b = g_find(L, b, cap, bad);
    if (a == b || bad) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(L + a, b);   // device scope
    if (old == a) return;
    a = old;
  }
  bad = 1;
}

// the half of the neighbourhood that precedes a voxel in flat order: 3 of 6, 13 of 26
__constant__ const signed char kCcBack[13][3] = {{0, 0, -1},  {0, -1, 0},  {-1, 0, 0},  {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1},
                                                 {-1, -1, 0}, {-1, 1, 0}, {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

template <int CONN>
__global__ void __launch_bounds__(kCcThreads) cc_merge_kernel(int* __restrict__ labels, CcAcc* __restrict__ acc, CcGeom g) {
  constexpr int NB = CONN == 6 ? 3 : 13;
  const int tid = threadIdx.x;
  const int per_vol = g.tz * g.ty * g.tx;
  const int vol = blockIdx.x / per_vol;
  int t = blockIdx.x - vol * per_vol;
  const int bx = t % g.tx;
  t /= g.tx;
  const int by = t % g.ty, bz = t / g.ty;
  int* __restrict__ L = labels + (int64_t)vol * g.nvox;
  const uint32_t cap = (uint32_t)g.nvox;
  int bad = 0;
  for (int k = 0; k < kCcPerThread; ++k) {
    const int i = tid + k * kCcThreads, lx = i & 31, ly = (i >> 5) & 7, lz = i >> 8;
    const bool face = lx == 0 || ly == 0 || lz == 0 || (CONN == 26 && (lx == kCcTX - 1 || ly == kCcTY - 1));
    const int z = bz * kCcTZ + lz, y = by * kCcTY + ly, x = bx * kCcTX + lx;
    if (!face || z >= g.Ds || y >= g.Hs || x >= g.Ws) continue;
    const int64_t fi = ((int64_t)z * g.Hs + y) * g.Ws + x;
    if (g_load(L + fi) < 0) continue;
    const bool left = lx > 0 && g_load(L + fi - 1) >= 0;   // the voxel before this one, in this tile, is foreground
    for (int d = 0; d < NB; ++d) {
      const int dz = kCcBack[d][0], dy = kCcBack[d][1], dx = kCcBack[d][2];
      const int nz = z + dz, ny = y + dy, nx = x + dx;
      if (nz < 0 || ny < 0 || ny >= g.Hs || nx < 0 || nx >= g.Ws) continue;
      const int nlx = lx + dx, nly = ly + dy;
      if (lz + dz >= 0 && nly >= 0 && nly < kCcTY && nlx >= 0 && nlx < kCcTX) continue;   // the same tile: (1) did it
      const int64_t fn = ((int64_t)nz * g.Hs + ny) * g.Ws + nx;
      if (g_load(L + fn) < 0) continue;
      // The neighbour lies in this tile's column of tiles (the seam is crossed along y or z) and not at its first x: the voxel before
      // this one has the voxel before the neighbour as its own neighbour across the same seam and does the union, and each of the two
      // pairs along x is one set since (1).
      if (left && nlx >= 1 && nlx < kCcTX && g_load(L + fn - 1) >= 0) continue;
      g_unite(L, (int)fi, (int)fn, cap, bad);
    }
  }
  if (bad) atomicOr(&acc[vol].status, kCcBadMerge);
}

__global__ void __launch_bounds__(kCcThreads) cc_flatten_kernel(int* __restrict__ labels, CcAcc* __restrict__ acc, int64_t nvox, int64_t total) {
  const uint32_t cap = (uint32_t)nvox;
  for (int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCcThreads) {
    const int64_t vol = i / nvox;
    int* __restrict__ L = labels + vol * nvox;
    const int l = g_load(labels + i);
    if (l < 0) continue;
    int bad = 0;
    const int r = g_find(L, l, cap, bad);
    if (r != l) atomicMin(labels + i, r);   // another workgroup may be descending through this word
    if (bad) atomicOr(&acc[vol].status, kCcBadFlatten);
  }
}

// ------------------------------------------------------------------------------------------
// (4) count.  A workgroup owns 4096 consecutive voxels of one volume, 16 per thread in registers.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcThreads) cc_count_kernel(const int* __restrict__ labels, int* __restrict__ size, int64_t nvox, int per_vol) {
  __shared__ int dom, dom_n;
  const int tid = threadIdx.x, lane = lane_id();
  const int vol = blockIdx.x / per_vol, part = blockIdx.x - vol * per_vol;
  const int64_t beg = (int64_t)part * kCcCountChunk;
  const int* __restrict__ L = labels + (int64_t)vol * nvox;
  int* __restrict__ sz = size + (int64_t)vol * nvox;
  if (tid == 0) dom = 0x7fffffff, dom_n = 0;
  int l[16], mn = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t i = beg + k * kCcThreads + tid;
    l[k] = i < nvox ? L[i] : -1;
    if (l[k] >= 0) mn = min(mn, l[k]);
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) mn = min(mn, __shfl_xor(mn, d));
  __syncthreads();
  if (lane == 0 && mn != 0x7fffffff) atomicMin(&dom, mn);
  __syncthreads();
  const int dr = dom;   // the workgroup's dominant root: its smallest
  int nd = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (l[k] == dr) ++nd, l[k] = -1;
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) nd += __shfl_xor(nd, d);
  if (lane == 0 && nd) atomicAdd(&dom_n, nd);
  // the other roots: lanes of the wave that hold the same root in slot k add once
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int v = l[k];
    unsigned long long pending = __ballot(v >= 0);
    while (pending) {   // every round retires at least the leader: at most 64 rounds
      const int leader = __ffsll((long long)pending) - 1;
      const int lv = __shfl(v, leader);
      const unsigned long long same = __ballot(v == lv);
      if (lane == leader) atomicAdd(sz + lv, __popcll(same));
      pending &= ~same;
    }
  }
  __syncthreads();
  if (tid == 0 && dom_n) atomicAdd(sz + dr, dom_n);
}

// ------------------------------------------------------------------------------------------
// (5) pick.  size[i] > 0 exactly where i is a root.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcThreads) cc_pick_kernel(const int* __restrict__ size, CcAcc* __restrict__ acc, int64_t nvox, int per_vol, int min_voxels) {
  __shared__ unsigned long long sbest;
  __shared__ int sn, sk, sv;
  const int tid = threadIdx.x, lane = lane_id();
  const int vol = blockIdx.x / per_vol, part = blockIdx.x - vol * per_vol;
  const int* __restrict__ sz = size + (int64_t)vol * nvox;
  if (tid == 0) sbest = 0, sn = 0, sk = 0, sv = 0;
  unsigned long long best = 0;
  int n = 0, nk = 0, nv = 0;
  for (int64_t i = (int64_t)part * kCcThreads + tid; i < nvox; i += (int64_t)per_vol * kCcThreads) {
    const int s = sz[i];
    if (s <= 0) continue;
    const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)(0x7fffffff - (int)i);   // a tie goes to the smaller root
    best = key > best ? key : best;
    ++n;
    if (s >= min_voxels) ++nk, nv += s;
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o > best ? o : best;
    n += __shfl_xor(n, d), nk += __shfl_xor(nk, d), nv += __shfl_xor(nv, d);
  }
  __syncthreads();
  if (lane == 0 && n) {
    atomicMax(&sbest, best);
    atomicAdd(&sn, n), atomicAdd(&sk, nk), atomicAdd(&sv, nv);
  }
  __syncthreads();
  if (tid == 0 && sn) {   // one set of global atomics per workgroup
    atomicMax(&acc[vol].best, sbest);
    atomicAdd(&acc[vol].ncomp, sn);
    if (sk) atomicAdd(&acc[vol].nkept, sk), atomicAdd(&acc[vol].kept_vox, sv);
  }
}

// ------------------------------------------------------------------------------------------
// (6) table
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcThreads) cc_table_kernel(const CcAcc* __restrict__ acc, int4* __restrict__ comps, int nvol, int keep) {
  const int v = blockIdx.x * kCcThreads + threadIdx.x;
  if (v >= nvol) return;
  const CcAcc a = acc[v];
  const int root = a.ncomp ? 0x7fffffff - (int)(uint32_t)(a.best & 0xffffffffu) : -1, big = (int)(a.best >> 32);
  const bool by_size = keep == XVIT_CC_MIN_VOXELS && a.nkept > 0;   // else the largest alone
  comps[2 * v] = int4{a.ncomp, root, big, by_size ? a.nkept : (a.ncomp ? 1 : 0)};
  comps[2 * v + 1] = int4{by_size ? a.kept_vox : big, a.status, 0, 0};
}

// ------------------------------------------------------------------------------------------
// (7) boxes over the kept voxels: volume_bbox.hip's chunks and partial records
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBoxThreads) cc_box_kernel(const int* __restrict__ labels, const int* __restrict__ size, const int4* __restrict__ comps,
                                                             int4* __restrict__ partial, int64_t nvox, int per_vol, int64_t chunk, int Ds, int Hs, int Ws,
                                                             int keep, int min_voxels) {
  __shared__ int4 red[2 * kBoxWaves];
  const int tid = threadIdx.x;
  const int vol = blockIdx.x / per_vol, part = blockIdx.x - vol * per_vol;
  const int64_t beg = (int64_t)part * chunk;
  const int64_t len = max((int64_t)0, min(nvox, beg + chunk) - beg);
  const int* __restrict__ L = labels + (int64_t)vol * nvox + beg;
  const int* __restrict__ sz = size + (int64_t)vol * nvox;
  const int4 c = comps[2 * vol];
  const int big_root = c.y;
  const bool by_size = keep == XVIT_CC_MIN_VOXELS && c.z >= min_voxels;   // some component qualifies exactly when the largest does
  Box b = empty_box(Ds, Hs, Ws);
  for (int64_t i = tid; i < len; i += kBoxThreads) {
    const int l = L[i];
    if (l < 0) continue;
    const bool kept = by_size ? sz[l] >= min_voxels : l == big_root;
    add_run<1>(b, (uint32_t)kept, (uint32_t)(beg + i), Hs, Ws);
  }
  b = block_merge(b, red);
  if (tid == 0) {
    partial[2 * (int64_t)blockIdx.x] = int4{b.z0, b.z1, b.y0, b.y1};
    partial[2 * (int64_t)blockIdx.x + 1] = int4{b.x0, b.x1, b.n, 0};
  }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
static int64_t cc_workspace_bytes(int nvol, int64_t nvox) {
  return cc_acc_bytes(nvol) + cc_size_bytes(nvol, nvox) + xvit_volume_bbox_workspace_bytes(nvol, nvox);
}

static int components_check(const char* who, const void* src, int src_dtype, int nvol, int Ds, int Hs, int Ws, const xvit_component_config* cfg, const int32_t* labels,
                            const int32_t* comps, const void* workspace, int64_t workspace_bytes) {
  XVIT_REQUIRE(src && cfg && labels && comps && workspace, "%s: null source, config, labels, comps or workspace", who);
  XVIT_REQUIRE(src_dtype == XVIT_I16 || src_dtype == XVIT_BF16 || src_dtype == XVIT_F32, "%s: unknown source dtype %d", who, src_dtype);
  XVIT_REQUIRE(cfg->connectivity == 6 || cfg->connectivity == 26, "%s: connectivity %d must be 6 or 26", who, cfg->connectivity);
  XVIT_REQUIRE(cfg->keep == XVIT_CC_LARGEST || cfg->keep == XVIT_CC_MIN_VOXELS, "%s: unknown keep mode %d", who, cfg->keep);
  XVIT_REQUIRE(cfg->min_voxels >= 1, "%s: min_voxels=%d must be >= 1", who, cfg->min_voxels);
  XVIT_REQUIRE(!isnan(cfg->foreground_above), "%s: foreground_above is NaN", who);
  XVIT_REQUIRE(nvol > 0 && Ds > 0 && Hs > 0 && Ws > 0, "%s: nvol=%d and the sizes (%d, %d, %d) must be positive", who, nvol, Ds, Hs, Ws);
  const int64_t nvox = (int64_t)Ds * Hs * Ws;
  XVIT_REQUIRE(nvox < (1ll << 31), "%s: a volume must have fewer than 2^31 voxels, got %lld", who, (long long)nvox);
  const int64_t tiles = (int64_t)((Ds + kCcTZ - 1) / kCcTZ) * ((Hs + kCcTY - 1) / kCcTY) * ((Ws + kCcTX - 1) / kCcTX);
  XVIT_REQUIRE(tiles * nvol < (1ll << 31) && ((nvox + kCcCountChunk - 1) / kCcCountChunk) * nvol < (1ll << 31), "%s: too many tiles for one launch", who);
  XVIT_REQUIRE(((uintptr_t)src & (src_dtype == XVIT_F32 ? 3 : 1)) == 0, "%s: the source is not aligned to its element size", who);
  XVIT_REQUIRE(((uintptr_t)labels & 15) == 0 && ((uintptr_t)comps & 15) == 0, "%s: labels and comps must be 16-byte aligned", who);
  XVIT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  XVIT_REQUIRE(workspace_bytes >= cc_workspace_bytes(nvol, nvox), "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
               (long long)cc_workspace_bytes(nvol, nvox));
  return XVIT_OK;
}

// launches (0) .. (6)
static void components_launch(const void* src, int src_dtype, int nvol, int Ds, int Hs, int Ws, const xvit_component_config& cfg, int32_t* labels, int32_t* comps,
                              void* workspace, hipStream_t s) {
  CcGeom g{Ds, Hs, Ws, (Ds + kCcTZ - 1) / kCcTZ, (Hs + kCcTY - 1) / kCcTY, (Ws + kCcTX - 1) / kCcTX, (int64_t)Ds * Hs * Ws};
  CcAcc* acc = (CcAcc*)workspace;
  int* size = (int*)((char*)workspace + cc_acc_bytes(nvol));
  const int64_t n16 = (cc_acc_bytes(nvol) + cc_size_bytes(nvol, g.nvox)) / 16;
  const unsigned tiles = (unsigned)((int64_t)nvol * g.tz * g.ty * g.tx);
  const int count_parts = (int)((g.nvox + kCcCountChunk - 1) / kCcCountChunk);
  const int pick_parts = (int)min((int64_t)max(1, 2048 / nvol), (g.nvox + 4 * kCcThreads - 1) / (4 * kCcThreads));
  hipLaunchKernelGGL(cc_zero_kernel, dim3(grid_for(n16, kCcThreads)), dim3(kCcThreads), 0, s, (int4*)workspace, n16);
  by_src_dtype(src_dtype, [&](auto t) {
    using S = decltype(t);
    if (cfg.connectivity == 6) hipLaunchKernelGGL((cc_tile_kernel<S, 6>), dim3(tiles), dim3(kCcThreads), 0, s, (const S*)src, labels, acc, g, cfg.foreground_above);
    else hipLaunchKernelGGL((cc_tile_kernel<S, 26>), dim3(tiles), dim3(kCcThreads), 0, s, (const S*)src, labels, acc, g, cfg.foreground_above);
  });
  if (cfg.connectivity == 6) hipLaunchKernelGGL(cc_merge_kernel<6>, dim3(tiles), dim3(kCcThreads), 0, s, labels, acc, g);
  else hipLaunchKernelGGL(cc_merge_kernel<26>, dim3(tiles), dim3(kCcThreads), 0, s, labels, acc, g);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for((int64_t)nvol * g.nvox, kCcThreads, 16384)), dim3(kCcThreads), 0, s, labels, acc, g.nvox, (int64_t)nvol * g.nvox);
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)((int64_t)nvol * count_parts)), dim3(kCcThreads), 0, s, (const int*)labels, size, g.nvox, count_parts);
  hipLaunchKernelGGL(cc_pick_kernel, dim3((unsigned)(nvol * pick_parts)), dim3(kCcThreads), 0, s, (const int*)size, acc, g.nvox, pick_parts, cfg.min_voxels);
  hipLaunchKernelGGL(cc_table_kernel, dim3((nvol + kCcThreads - 1) / kCcThreads), dim3(kCcThreads), 0, s, (const CcAcc*)acc, (int4*)comps, nvol, cfg.keep);
}

}  // namespace xvit

extern "C" int64_t xvit_volume_components_workspace_bytes(int nvol, int64_t nvox) {
  if (nvol <= 0 || nvox <= 0) return 0;
  return xvit::cc_workspace_bytes(nvol, nvox);
}

extern "C" int xvit_volume_components(const void* src, int src_dtype, int nvol, int Ds, int Hs, int Ws, const xvit_component_config* cfg, int32_t* labels,
                                      int32_t* comps, void* workspace, int64_t workspace_bytes, xvit_stream_t stream) {
  const int rc = xvit::components_check("xvit_volume_components", src, src_dtype, nvol, Ds, Hs, Ws, cfg, labels, comps, workspace, workspace_bytes);
  if (rc != XVIT_OK) return rc;
  xvit::components_launch(src, src_dtype, nvol, Ds, Hs, Ws, *cfg, labels, comps, workspace, (hipStream_t)stream);
  return xvit::check_launch("xvit_volume_components");
}

extern "C" int xvit_volume_bbox_components(const void* src, int src_dtype, int nvol, int M, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config* cfg,
                                           const xvit_component_config* comp, int32_t* boxes, int32_t* crop, float* params, int32_t* labels, int32_t* comps,
                                           void* workspace, int64_t workspace_bytes, xvit_stream_t stream) {
  const char* who = "xvit_volume_bbox_components";
  XVIT_REQUIRE(cfg && boxes && crop, "%s: null crop config, boxes or crop", who);
  const int rc = xvit::components_check(who, src, src_dtype, nvol, Ds, Hs, Ws, comp, labels, comps, workspace, workspace_bytes);
  if (rc != XVIT_OK) return rc;
  XVIT_REQUIRE(cfg->mode == XVIT_CROP_BOXES_ONLY || cfg->mode == XVIT_CROP_CENTER || cfg->mode == XVIT_CROP_FIT, "%s: unknown mode %d", who, cfg->mode);
  XVIT_REQUIRE(M > 0 && nvol % M == 0, "%s: nvol=%d must be a positive multiple of M=%d > 0", who, nvol, M);
  XVIT_REQUIRE(D > 0 && H > 0 && W > 0, "%s: destination sizes (%d, %d, %d) must be positive", who, D, H, W);
  XVIT_REQUIRE(cfg->margin[0] >= 0 && cfg->margin[1] >= 0 && cfg->margin[2] >= 0, "%s: margin (%d, %d, %d) must be >= 0", who, cfg->margin[0], cfg->margin[1],
               cfg->margin[2]);
  XVIT_REQUIRE(!isnan(cfg->foreground_above) && cfg->foreground_above == comp->foreground_above, "%s: the two configs must hold the same foreground_above, not NaN", who);
  XVIT_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)crop & 15) == 0, "%s: boxes and crop must be 16-byte aligned", who);
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "%s: the parameter table must be 16-byte aligned", who);
  const hipStream_t s = (hipStream_t)stream;
  const int64_t nvox = (int64_t)Ds * Hs * Ws;
  xvit::components_launch(src, src_dtype, nvol, Ds, Hs, Ws, *comp, labels, comps, workspace, s);
  int64_t chunk;
  const int per_vol = xvit::bbox_parts(nvol, nvox, &chunk);
  const int* size = (const int*)((char*)workspace + xvit::cc_acc_bytes(nvol));
  int4* partial = (int4*)((char*)workspace + xvit::cc_acc_bytes(nvol) + xvit::cc_size_bytes(nvol, nvox));
  hipLaunchKernelGGL(xvit::cc_box_kernel, dim3((unsigned)((int64_t)nvol * per_vol)), dim3(xvit::kBoxThreads), 0, s, (const int*)labels, size, (const int4*)comps, partial,
                     nvox, per_vol, chunk, Ds, Hs, Ws, comp->keep, comp->min_voxels);
  xvit::launch_volume_bbox_finish(partial, nvol, M, per_vol, Ds, Hs, Ws, D, H, W, *cfg, (int4*)boxes, (int4*)crop, params, s);
  return xvit::check_launch(who);
}
