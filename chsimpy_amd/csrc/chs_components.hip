// chs_components.hip -- connected components of the thresholded field on the device: droplet count, sizes, bounding
// boxes, spanning (the definition: include/chs_hip.h, chs_components).
//
// A union-find forest over the pixels, built by atomic minima (chs_cc_host.h: find, unite -- with the termination and
// stale-read arguments), in phases that are separate launches: no workgroup ever waits for another one, nothing is
// polled, and what a phase needs of the one before it is fresh because a kernel boundary lies between them.
//   1  k_cc_tile     a workgroup thresholds one CHS_CC_TR x CHS_CC_TC tile into LDS (16-byte loads where N allows),
//                    unites every foreground pixel with its earlier neighbours inside the tile (LDS atomicMin), flattens
//                    and writes L[p] = the global index of p's tile root, -1 for background
//   2  k_cc_merge    one thread per pixel of every tile's first row and first column unites it in L with its neighbours
//                    in the adjacent (and, for connectivity 8, the diagonal) tiles: device-scope atomicMin, the ONLY
//                    writes to L in this launch -- no path compression by plain stores
//   3  k_cc_flatten  L[p] = root(p)
//   4  k_cc_count, k_cc_scan, k_cc_scatter   the roots (L[p] == p) numbered by ascending index: counts per block of
//                    CHS_CC_NUM_BLOCK pixels, one workgroup scanning the counts, then id[root] and the table rows' start
//                    values.  (The host reads the count between scan and scatter: the table is grown to it.)
//   5  k_cc_stats    area and bounding box by integer atomics into the table row id[L[p]], runs of equal labels combined
//                    in the wavefront and the labels of a workgroup's tile in LDS first; the same sweep VERIFIES the
//                    labelling: equal labels across every joined pair (right, lower, lower diagonals), L[L[p]] == L[p],
//                    L[p] <= p.  Violations are counted into one word.
//   6  k_cc_summary  the seven words from the table, a fixed tree over integers
// Visibility (phase 2): the per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another
// CU's stores, so a load of L there -- plain or L1-bypassing -- may return any earlier value of the word.  The algorithm
// is correct under exactly that assumption: every earlier value is a smaller-or-equal pixel of the same component, and
// whether a pixel is a root is decided by what the atomicMin returns (chs_cc_host.h).  Every loop has a cap it cannot
// reach; one that reaches it sets a bit of the error word and leaves.  A nonzero error word or violation count makes the
// look return CHS_ECHECK.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "chs_look.h"
#include "chs_cc_host.h"

#define CC_THREADS 256
#define CC_WAVES (CC_THREADS / CHS_WAVE)
#define CC_PIX (CHS_CC_TILE / CC_THREADS)            // pixels of a thread in k_cc_tile
#define CC_ITERS (CHS_CC_NUM_BLOCK / CC_THREADS)     // pixels of a thread in the numbering
#define CC_SLOT_BITS 10
#define CC_SLOTS (1 << CC_SLOT_BITS)                 // labels a workgroup of k_cc_stats combines in LDS
#define CC_SCAN_THREADS 1024
#define CC_SUM_BLOCKS 1024
// the words of a look
#define CC_W_ERR 0
#define CC_W_VIOL 1
#define CC_W_COUNT 2
#define CC_NW 4

static_assert(CHS_CC_TILE % CC_THREADS == 0 && CHS_CC_NUM_BLOCK % CC_THREADS == 0, "whole pixels per thread");
static_assert(CHS_CC_TC % 4 == 0, "a 16-byte load stays inside a tile row");
static_assert(CC_ITERS * CC_WAVES == CHS_WAVE, "k_cc_scatter scans its (iteration, wavefront) counts in one wavefront");

typedef long long cc_i64;
static_assert(sizeof(cc_i64) == sizeof(int64_t) && sizeof(chs_cc::Summary) == CHS_CC_WORDS * sizeof(int64_t), "the summary is the seven int64 words");

// how find / unite read and min-update a label word (chs_cc_host.h): the tile's words in LDS ...
struct CcLdsWords {
  int* w;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int amin(int i, int v) const { return atomicMin(w + i, v); }
};
// ... and L in global memory: a load that bypasses this CU's L1 (it may still be an earlier value: the header's
// argument), and the device-scope atomic minimum
struct CcGlobalWords {
  int* w;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int amin(int i, int v) const { return atomicMin(w + i, v); }
};

// ---- phase 1 ---------------------------------------------------------------------------------------------------------
// grid (column tiles, row tiles).  V: pixels per load (16 bytes where N is a multiple of V, else 1).  A thread owns the
// CC_PIX pixels k = (it CC_THREADS + tid) V + e of the tile, it < CC_PIX / V, e < V.  No load is guarded by a branch: a
// pixel outside the grid is clamped to one inside and masked.
template <typename T, int V, bool NT>
__global__ __launch_bounds__(CC_THREADS) void k_cc_tile(const void* Uv, int N, double t, int conn, int above,
                                                        int* __restrict__ L, int* __restrict__ words) {
  __shared__ int par[CHS_CC_TILE];
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int tid = threadIdx.x, i0 = blockIdx.y * CHS_CC_TR, j0 = blockIdx.x * CHS_CC_TC;
  unsigned fg = 0, in = 0;   // bit it V + e: the pixel is foreground / inside the grid
#pragma unroll
  for (int it = 0; it < CC_PIX / V; ++it) {
    const int k = (it * CC_THREADS + tid) * V;
    const int i = i0 + k / CHS_CC_TC, j = j0 + k % CHS_CC_TC;
    const bool inside = i < N && j < N;   // (V > 1: N and j are multiples of V, so j < N is j + V - 1 < N)
    const T CHS_GLOBAL* src = U + (size_t)(i < N ? i : N - 1) * N + (j < N ? j : N - V);
    T x[V];
    chs_load<T, V, NT>(src, x);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool f = inside && chs_cc::fg_of((double)x[e], t, above);
      par[k + e] = f ? k + e : -1;
      fg |= (f ? 1u : 0u) << (it * V + e);
      in |= (inside ? 1u : 0u) << (it * V + e);
    }
  }
  __syncthreads();
  CcLdsWords a{par};
  int err = 0;
#pragma unroll 1
  for (int b = 0; b < CC_PIX; ++b) {
    if (!((fg >> b) & 1u)) continue;
    const int k = ((b / V) * CC_THREADS + tid) * V + b % V;
    int q[4];
    const int n = chs_cc::tile_pairs(conn, k / CHS_CC_TC, k % CHS_CC_TC, q);
    for (int s = 0; s < n; ++s)
      if (a.load(q[s]) >= 0)   // (foreground or not: that never changes)
        chs_cc::unite(a, k, q[s], CHS_CC_TILE, &err, CHS_CC_ERR_TILE_FIND, CHS_CC_ERR_TILE_UNITE);
  }
  __syncthreads();
#pragma unroll 1
  for (int b = 0; b < CC_PIX; ++b) {
    if (!((in >> b) & 1u)) continue;
    const int k = ((b / V) * CC_THREADS + tid) * V + b % V;
    int l = -1;
    if ((fg >> b) & 1u) {
      const int r = chs_cc::find(a, k, CHS_CC_TILE, &err, CHS_CC_ERR_TILE_FIND);
      l = (i0 + r / CHS_CC_TC) * N + j0 + r % CHS_CC_TC;
    }
    L[(size_t)(i0 + k / CHS_CC_TC) * N + j0 + k % CHS_CC_TC] = l;
  }
  if (err) atomicOr(&words[CC_W_ERR], err);
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------
// One thread per border position of every tile (chs_cc_host.h: border_pairs).
__global__ __launch_bounds__(CC_THREADS) void k_cc_merge(int* L, int N, int conn, int tx, int ntiles, int* __restrict__ words) {
  const int g = blockIdx.x * CC_THREADS + threadIdx.x;
  const int tile = g / CHS_CC_BORDER, k = g % CHS_CC_BORDER;
  if (tile >= ntiles) return;
  int p = 0, q[3];
  const int n = chs_cc::border_pairs(N, conn, tile / tx, tile % tx, k, &p, q);
  if (n == 0) return;
  CcGlobalWords a{L};
  if (a.load(p) < 0) return;
  int err = 0;
  for (int s = 0; s < n; ++s)
    if (a.load(q[s]) >= 0)
      chs_cc::unite(a, p, q[s], N * N, &err, CHS_CC_ERR_MERGE_FIND, CHS_CC_ERR_MERGE_UNITE);
  if (err) atomicOr(&words[CC_W_ERR], err);
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------
// L[p] = root(p).  The words this launch reads are those of phase 2 (fresh: the kernel boundary) or roots written here.
__global__ __launch_bounds__(CC_THREADS) void k_cc_flatten(int* L, int n2, int* __restrict__ words) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= n2) return;
  CcGlobalWords a{L};
  const int l = a.load(p);
  if (l < 0 || l == p) return;
  int err = 0;
  const int r = chs_cc::find(a, l, n2, &err, CHS_CC_ERR_FLATTEN);
  if (r != l) L[p] = r;
  if (err) atomicOr(&words[CC_W_ERR], err);
}

// ---- phase 4 ---------------------------------------------------------------------------------------------------------
// A block numbers the CHS_CC_NUM_BLOCK pixels from blockIdx.x * CHS_CC_NUM_BLOCK on; its pixel (it, tid) is
// base + it * CC_THREADS + tid, so ascending (it, wavefront, lane) is ascending index.
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(const int* __restrict__ L, int n2, int* __restrict__ cnt) {
  __shared__ int red[CC_WAVES];
  const int base = blockIdx.x * CHS_CC_NUM_BLOCK;
  int c = 0;
#pragma unroll
  for (int it = 0; it < CC_ITERS; ++it) {
    const int p = base + it * CC_THREADS + threadIdx.x;
    c += (p < n2 && L[p < n2 ? p : 0] == p) ? 1 : 0;
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) c += __shfl_down(c, off, CHS_WAVE);
  if ((threadIdx.x & (CHS_WAVE - 1)) == 0) red[threadIdx.x / CHS_WAVE] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < CC_WAVES; ++w) s += red[w];
    cnt[blockIdx.x] = s;
  }
}

// cnt[b] <- the sum of the counts before b; words[CC_W_COUNT] <- their total.  One workgroup.
__global__ __launch_bounds__(CC_SCAN_THREADS) void k_cc_scan(int* __restrict__ cnt, int nblk, int* __restrict__ words) {
  __shared__ int s[CC_SCAN_THREADS];
  const int tid = threadIdx.x, per = (nblk + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
  const int b0 = tid * per, b1 = (b0 + per < nblk) ? b0 + per : nblk;
  int own = 0;
  for (int b = b0; b < b1; ++b) own += cnt[b];
  s[tid] = own;
  __syncthreads();
#pragma unroll 1
  for (int off = 1; off < CC_SCAN_THREADS; off <<= 1) {
    const int v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int run = s[tid] - own;
  for (int b = b0; b < b1; ++b) {
    const int c = cnt[b];
    cnt[b] = run;
    run += c;
  }
  if (tid == CC_SCAN_THREADS - 1) words[CC_W_COUNT] = s[tid];
}

// id[root] <- its number; the table row of that number <- first, and the start values of the statistics: area 0, and the
// bounding box of the first pixel alone (it is the component's smallest index, so its row is imin already).
__global__ __launch_bounds__(CC_THREADS) void k_cc_scatter(const int* __restrict__ L, int n2, int N, const int* __restrict__ off,
                                                           int* __restrict__ id, int* __restrict__ table) {
  __shared__ int pre[CC_ITERS * CC_WAVES];
  const int base = blockIdx.x * CHS_CC_NUM_BLOCK, lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  unsigned flags = 0;
#pragma unroll
  for (int it = 0; it < CC_ITERS; ++it) {
    const int p = base + it * CC_THREADS + threadIdx.x;
    const bool f = p < n2 && L[p < n2 ? p : 0] == p;
    flags |= (f ? 1u : 0u) << it;
    const unsigned long long m = __ballot(f);
    if (lane == 0) pre[it * CC_WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  if (wave == 0) {   // the exclusive scan of the CC_ITERS * CC_WAVES = 64 counts, in one wavefront
    const int own = pre[lane];
    int v = own;
#pragma unroll
    for (int o = 1; o < CHS_WAVE; o <<= 1) {
      const int u = __shfl_up(v, o, CHS_WAVE);
      if (lane >= o) v += u;
    }
    pre[lane] = v - own;
  }
  __syncthreads();
  const int first = off[blockIdx.x];
#pragma unroll
  for (int it = 0; it < CC_ITERS; ++it) {
    const bool f = (flags >> it) & 1u;
    const unsigned long long m = __ballot(f);
    if (f) {
      const int p = base + it * CC_THREADS + threadIdx.x;
      const int row = first + pre[it * CC_WAVES + wave] + __popcll(m & ((1ull << lane) - 1ull));
      const int i = p / N, j = p - i * N;
      id[p] = row;
      int* r = table + (size_t)row * CHS_CC_COLS;
      r[0] = p; r[1] = 0; r[2] = i; r[3] = i; r[4] = j; r[5] = j;
    }
  }
}

// ---- phase 5 ---------------------------------------------------------------------------------------------------------
// grid (column tiles, row tiles): a workgroup sweeps one CHS_CC_TR x CHS_CC_TC tile, a wavefront one tile row per
// iteration -- a small component lies in one tile or a few, so nearly all of what it adds meets in one workgroup.  A run
// of equal labels inside a wavefront's row is one contribution (area = its length, its row, its first and last column),
// made by the run's first lane.  The contributions go to an LDS slot chosen by the label where the slot is free or holds
// that label, and straight to the table otherwise; the slots are added to the table at the end, so a component costs a
// workgroup four global atomics, not four per run.  Integer atomics: the table does not depend on their order.
__global__ __launch_bounds__(CC_THREADS) void k_cc_stats(const int* __restrict__ L, const int* __restrict__ id, int N,
                                                         int conn, int C, int* __restrict__ table, int* __restrict__ words) {
  __shared__ int key[CC_SLOTS], sArea[CC_SLOTS], sImax[CC_SLOTS], sJmin[CC_SLOTS], sJmax[CC_SLOTS];
  static_assert(CHS_CC_TC == CHS_WAVE && CHS_CC_TR % CC_WAVES == 0, "a wavefront sweeps whole tile rows");
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = blockIdx.x * CHS_CC_TC + lane;
  for (int s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) {
    key[s] = -1; sArea[s] = 0; sImax[s] = -1; sJmin[s] = INT_MAX; sJmax[s] = -1;
  }
  __syncthreads();
  int viol = 0;
#pragma unroll 1
  for (int it = 0; it < CHS_CC_TR / CC_WAVES; ++it) {
    const int i = blockIdx.y * CHS_CC_TR + it * CC_WAVES + wave;
    const bool inb = i < N && j < N;
    const int p = i * N + j;
    const int l = inb ? L[p] : -2;
    if (l >= 0) {   // the checks of the labelling
      viol += (L[l] != l) ? 1 : 0;
      viol += (l > p) ? 1 : 0;
      const bool right = j + 1 < N, down = i + 1 < N;
      if (right) { const int o = L[p + 1]; viol += (o >= 0 && o != l) ? 1 : 0; }
      if (down) {
        const int o = L[p + N];
        viol += (o >= 0 && o != l) ? 1 : 0;
        if (conn == 8) {
          if (j > 0) { const int d = L[p + N - 1]; viol += (d >= 0 && d != l) ? 1 : 0; }
          if (right) { const int d = L[p + N + 1]; viol += (d >= 0 && d != l) ? 1 : 0; }
        }
      }
    }
    // the runs: every lane takes part in the two cross-lane operations
    const int before = __shfl_up(l, 1, CHS_WAVE);
    const bool head = lane == 0 || before != l;
    const unsigned long long heads = __ballot(head);
    const unsigned long long rest = lane == CHS_WAVE - 1 ? 0ull : heads >> (lane + 1);
    const int len = rest ? __ffsll((long long)rest) : CHS_WAVE - lane;
    if (head && l >= 0) {
      const unsigned slot = ((unsigned)l * 2654435761u) >> (32 - CC_SLOT_BITS);
      const int was = atomicCAS(&key[slot], -1, l);
      if (was == -1 || was == l) {
        atomicAdd(&sArea[slot], len);
        atomicMax(&sImax[slot], i);
        atomicMin(&sJmin[slot], j);
        atomicMax(&sJmax[slot], j + len - 1);
      } else {
        const int row = id[l];
        if ((unsigned)row < (unsigned)C) {   // (a label that is no root has no number: counted above, never written)
          int* r = table + (size_t)row * CHS_CC_COLS;
          atomicAdd(&r[1], len);
          atomicMax(&r[3], i);
          atomicMin(&r[4], j);
          atomicMax(&r[5], j + len - 1);
        } else {
          ++viol;
        }
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) {
    const int l = key[s];
    const int row = l >= 0 ? id[l] : -1;
    if (l >= 0 && (unsigned)row >= (unsigned)C) ++viol;
    if ((unsigned)row < (unsigned)C) {
      int* r = table + (size_t)row * CHS_CC_COLS;
      atomicAdd(&r[1], sArea[s]);
      atomicMax(&r[3], sImax[s]);
      atomicMin(&r[4], sJmin[s]);
      atomicMax(&r[5], sJmax[s]);
    }
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) viol += __shfl_down(viol, off, CHS_WAVE);
  if (lane == 0 && viol) atomicAdd(&words[CC_W_VIOL], viol);
}

// ---- phase 6 ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ chs_cc::Summary cc_block_sum(chs_cc::Summary mine, chs_cc::Summary* red) {
  red[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int off = CC_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = chs_cc::summary_add(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

// part[block] <- the summary of the rows block, block + gridDim.x, ... (a thread adds its rows in ascending order)
__global__ __launch_bounds__(CC_THREADS) void k_cc_summary_rows(const int* __restrict__ table, int C, int N, chs_cc::Summary* __restrict__ part) {
  __shared__ chs_cc::Summary red[CC_THREADS];
  chs_cc::Summary s = chs_cc::summary_zero();
  for (int r = blockIdx.x * CC_THREADS + threadIdx.x; r < C; r += gridDim.x * CC_THREADS)
    s = chs_cc::summary_add(s, chs_cc::summary_of_row(table + (size_t)r * CHS_CC_COLS, N));
  s = cc_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_summary_fin(const chs_cc::Summary* __restrict__ part, int nparts, chs_cc::Summary* __restrict__ out) {
  __shared__ chs_cc::Summary red[CC_THREADS];
  chs_cc::Summary s = chs_cc::summary_zero();
  for (int r = threadIdx.x; r < nparts; r += CC_THREADS) s = chs_cc::summary_add(s, part[r]);
  s = cc_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// id[p] <- the number of p's component, -1 for background, in place: a root's entry is rewritten with itself.
__global__ __launch_bounds__(CC_THREADS) void k_cc_labels(const int* __restrict__ L, int* id, int n2) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= n2) return;
  const int l = L[p];
  const int v = l >= 0 ? id[l] : -1;
  if (l != p) id[p] = v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct CcResult {   // pinned
  int words[CC_NW];
  chs_cc::Summary out;
};

struct CcBuf : LookBase {   // have: L, id, table and count are the look's snapshot
  int nblk = 0;
  int* L = nullptr;             // [N * N] labels: the root's index, -1 for background
  int* id = nullptr;            // [N * N] the number at every root; the label image after k_cc_labels
  int* blk = nullptr;           // [nblk] the numbering's block counts, then offsets
  int* table = nullptr;         // [cap][CHS_CC_COLS]
  cc_i64 cap = 0;
  int* words = nullptr;         // [CC_NW]
  chs_cc::Summary* part = nullptr;   // [CC_SUM_BLOCKS]
  chs_cc::Summary* out = nullptr;    // [1]
  CcResult* hRes = nullptr;
  bool labelled = false;        // k_cc_labels has run behind it
  cc_i64 count = 0;
};

void cc_release(CcBuf* s) {
  if (!s) return;
  hipFree(s->L); hipFree(s->id); hipFree(s->blk); hipFree(s->table); hipFree(s->words); hipFree(s->part); hipFree(s->out);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int cc_alloc(CcBuf* s) {
  const int N = s->N;
  s->nblk = chs_cc::num_blocks(N);
  const size_t n2 = (size_t)N * N;
  CHS_HIP(hipMalloc(&s->L, sizeof(int) * n2));
  CHS_HIP(hipMalloc(&s->id, sizeof(int) * n2));
  CHS_HIP(hipMalloc(&s->blk, sizeof(int) * (size_t)s->nblk));
  CHS_HIP(hipMalloc(&s->words, sizeof(int) * CC_NW));
  CHS_HIP(hipMalloc(&s->part, sizeof(chs_cc::Summary) * CC_SUM_BLOCKS));
  CHS_HIP(hipMalloc(&s->out, sizeof(chs_cc::Summary)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(CcResult), hipHostMallocDefault));
  return CHS_OK;
}

template <typename T>
int launch_tile(const CcBuf* s, const void* U, double t, int conn, int side, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const int N = s->N;
  const dim3 grid(chs_cc::tiles_of(N, CHS_CC_TC), chs_cc::tiles_of(N, CHS_CC_TR));
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  const bool nt = chs_grid_exceeds_cache((size_t)N, sizeof(T));
  if (N % V == 0) {
    if (nt) k_cc_tile<T, V, true><<<grid, CC_THREADS, 0, st>>>(U, N, t, conn, side, s->L, s->words);
    else k_cc_tile<T, V, false><<<grid, CC_THREADS, 0, st>>>(U, N, t, conn, side, s->L, s->words);
  } else {
    if (nt) k_cc_tile<T, 1, true><<<grid, CC_THREADS, 0, st>>>(U, N, t, conn, side, s->L, s->words);
    else k_cc_tile<T, 1, false><<<grid, CC_THREADS, 0, st>>>(U, N, t, conn, side, s->L, s->words);
  }
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

std::string cc_failure(const int* w) {
  std::string m;
  const int e = w[CC_W_ERR];
  if (e & CHS_CC_ERR_TILE_FIND) m += " find in a tile reached its cap;";
  if (e & CHS_CC_ERR_TILE_UNITE) m += " unite in a tile reached its cap;";
  if (e & CHS_CC_ERR_MERGE_FIND) m += " find in the border merge reached its cap;";
  if (e & CHS_CC_ERR_MERGE_UNITE) m += " unite in the border merge reached its cap;";
  if (e & CHS_CC_ERR_FLATTEN) m += " find in the flatten pass reached its cap;";
  if (w[CC_W_VIOL]) m += " " + std::to_string(w[CC_W_VIOL]) + " violations of the labelling (joined pixels with unlike labels, a label that is no root or above its pixel);";
  return m;
}

// Phases 1 to 4b, the count read back; then 4c to 6.  Nothing of the handle is written and nothing the step loop owns is
// read (no state, no halt flag): its field alone.
int cc_run(CcBuf* s, Engine* E, hipStream_t st, double t, int conn, int side, const std::string& who) {
  const int N = s->N, n2 = N * N;
  const int tx = chs_cc::tiles_of(N, CHS_CC_TC), ntiles = tx * chs_cc::tiles_of(N, CHS_CC_TR);
  const int pixBlocks = (n2 + CC_THREADS - 1) / CC_THREADS;
  look_forget(s);
  s->labelled = false;
  CHS_HIP(hipMemsetAsync(s->words, 0, sizeof(int) * CC_NW, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  int rc = E->dtype == CHS_F64 ? launch_tile<double>(s, E->dU, t, conn, side, st) : launch_tile<float>(s, E->dU, t, conn, side, st);
  if (rc) return rc;
  if (ntiles > 1) {
    k_cc_merge<<<(ntiles * CHS_CC_BORDER + CC_THREADS - 1) / CC_THREADS, CC_THREADS, 0, st>>>(s->L, N, conn, tx, ntiles, s->words);
    CHS_HIP(hipGetLastError());
    k_cc_flatten<<<pixBlocks, CC_THREADS, 0, st>>>(s->L, n2, s->words);
    CHS_HIP(hipGetLastError());
  }
  k_cc_count<<<s->nblk, CC_THREADS, 0, st>>>(s->L, n2, s->blk);
  CHS_HIP(hipGetLastError());
  k_cc_scan<<<1, CC_SCAN_THREADS, 0, st>>>(s->blk, s->nblk, s->words);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * CC_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  if (s->hRes->words[CC_W_ERR]) { chs_set_error(who + ": self-check failed:" + cc_failure(s->hRes->words)); return CHS_ECHECK; }
  const cc_i64 C = s->hRes->words[CC_W_COUNT];
  if (C > s->cap) {   // the table grows to the count (and a little beyond: the next look of a coarsening run has fewer)
    CHS_HIP(hipFree(s->table));
    s->table = nullptr; s->cap = 0;
    const cc_i64 cap = C + C / 8 + 1024;
    CHS_HIP(hipMalloc(&s->table, sizeof(int) * CHS_CC_COLS * (size_t)cap));
    s->cap = cap;
  }
  if (C > 0) {
    k_cc_scatter<<<s->nblk, CC_THREADS, 0, st>>>(s->L, n2, N, s->blk, s->id, s->table);
    CHS_HIP(hipGetLastError());
    k_cc_stats<<<dim3(tx, ntiles / tx), CC_THREADS, 0, st>>>(s->L, s->id, N, conn, (int)C, s->table, s->words);
    CHS_HIP(hipGetLastError());
  }
  const int parts = C > 0 ? (int)std::min<cc_i64>((C + CC_THREADS - 1) / CC_THREADS, CC_SUM_BLOCKS) : 1;
  k_cc_summary_rows<<<parts, CC_THREADS, 0, st>>>(s->table, (int)C, N, s->part);
  CHS_HIP(hipGetLastError());
  k_cc_summary_fin<<<1, CC_THREADS, 0, st>>>(s->part, parts, s->out);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * CC_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(chs_cc::Summary), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  if (s->hRes->words[CC_W_ERR] || s->hRes->words[CC_W_VIOL]) {
    chs_set_error(who + ": self-check failed:" + cc_failure(s->hRes->words));
    return CHS_ECHECK;
  }
  s->count = C;
  return look_end(s);
}
}  // namespace

void chs_cc_free(void** buf) {
  if (!buf) return;
  cc_release((CcBuf*)*buf);
  *buf = nullptr;
}

void chs_cc_forget(void* buf) {
  if (!buf) return;
  CcBuf* s = (CcBuf*)buf;
  look_forget(s);
  s->labelled = false; s->count = 0;
}

int chs_cc_snapshot(const void* buf, ChsCcSnapshot* out, const char* who_) {
  const CcBuf* s = (const CcBuf*)buf;
  if (!s || !s->have) { chs_set_error(std::string(who_) + ": no components look to build on"); return CHS_ESTATE; }
  out->L = s->L; out->id = s->id; out->table = s->table; out->count = s->count; out->ms = s->ms;
  return CHS_OK;
}

int chs_cc_look(Engine* E, hipStream_t st, void** buf, double threshold, int32_t connectivity, int32_t side, int64_t* out,
                const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if (connectivity != 4 && connectivity != 8) { chs_set_error(who + ": the connectivity is 4 or 8"); return CHS_EINVAL; }
  if (side != CHS_CC_BELOW && side != CHS_CC_ABOVE) { chs_set_error(who + ": the side is CHS_CC_BELOW (0) or CHS_CC_ABOVE (1)"); return CHS_EINVAL; }
  if ((rc = look_check_field(E, CHS_CC_MAX_N, who))) return rc;
  if ((rc = look_buffers<CcBuf>(buf, E->N, cc_alloc, cc_release))) return rc;
  CcBuf* s = (CcBuf*)*buf;
  if ((rc = cc_run(s, E, st, threshold, connectivity, side, who))) return rc;
  memcpy(out, &s->hRes->out, sizeof(int64_t) * CHS_CC_WORDS);
  return CHS_OK;
}

int chs_cc_table(void* buf, int device, hipStream_t st, int64_t rows, int32_t* out, const char* who_) {
  const std::string who(who_);
  const CcBuf* s = (const CcBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (rows != s->count) { chs_set_error(who + ": rows = " + std::to_string(rows) + ", the last look counted " + std::to_string(s->count)); return CHS_EINVAL; }
  if (rows == 0) return CHS_OK;
  return look_fetch(device, st, out, s->table, sizeof(int32_t) * CHS_CC_COLS * (size_t)rows);
}

int chs_cc_labels(void* buf, int device, hipStream_t st, int32_t* out, const char* who_) {
  const std::string who(who_);
  CcBuf* s = (CcBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  CHS_HIP(hipSetDevice(device));
  const int n2 = s->N * s->N;
  if (!s->labelled) {
    k_cc_labels<<<(n2 + CC_THREADS - 1) / CC_THREADS, CC_THREADS, 0, st>>>(s->L, s->id, n2);
    CHS_HIP(hipGetLastError());
    s->labelled = true;
  }
  CHS_HIP(hipMemcpyAsync(out, s->id, sizeof(int32_t) * (size_t)n2, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  return CHS_OK;
}

extern "C" int chs_components(chs_handle h, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_CC_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_components: null handle"); return CHS_EINVAL; }
  return chs_cc_look(E, E->stream, &E->cc, threshold, connectivity, side, out, "chs_components");
}

extern "C" int chs_components_table(chs_handle h, int64_t rows, int32_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_components_table: null handle"); return CHS_EINVAL; }
  return chs_cc_table(E->cc, E->hc.device, E->stream, rows, out, "chs_components_table");
}

extern "C" int chs_components_labels(chs_handle h, int32_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_components_labels: null handle"); return CHS_EINVAL; }
  return chs_cc_labels(E->cc, E->hc.device, E->stream, out, "chs_components_labels");
}

extern "C" int chs_components_last_ms(chs_handle h, double* ms) {
  return look_last_ms(h, h ? (const CcBuf*)((Engine*)h)->cc : nullptr, ms, "chs_components");
}

extern "C" int chs_components_tile(int32_t* rows, int32_t* cols) {
  if (!rows || !cols) { chs_set_error("chs_components_tile: null argument"); return CHS_EINVAL; }
  *rows = CHS_CC_TR;
  *cols = CHS_CC_TC;
  return CHS_OK;
}
