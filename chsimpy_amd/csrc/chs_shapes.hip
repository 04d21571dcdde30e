// chs_shapes.hip -- the shape of every droplet on the device: counts of pixels, pairs and cells, wall edges, positional
// sums up to the second order and fixed-point sums of the composition, one int64 row per connected component (DESIGN.md
// section 3k; the definition: include/chs_hip.h, chs_shapes).
//
// A shapes look is a components look first: chs_cc_look labels the field on the handle's component buffers and leaves
// the root label of every pixel (L), the number at every root (id) and the component table there.  Then, here:
//   1  k_sh_init     a thread per row: `first` from the component table, every other cell 0
//   2  k_sh_sweep    one sweep over U, L and id.  A workgroup per CHS_CC_TR x CHS_CC_TC tile, a wavefront per tile row, a
//                    lane per pixel.  Everything a pixel adds to its own component is a predicate of the pixel and of five
//                    neighbour labels, so a run of equal labels inside the wavefront is ONE contribution, made by the
//                    run's first lane: the counts are population counts of ballots under the run's lane mask, the
//                    positional sums are closed forms of (row, first column, length), the two fixed-point sums come from a
//                    segmented suffix sum over the run's lanes.  The contribution goes to an LDS slot keyed by the label
//                    (64-bit LDS atomics) where the slot is free or holds that label, and straight to the table row
//                    id[label] (64-bit global atomics) otherwise; the slots are added to the table at the end.
//   3  k_sh_summary_rows, k_sh_summary_fin   the column sums, the holes and the wall-free components from the table
// Every cell is an integer and every accumulation an integer add: the table does not depend on the order of the atomics.
// The sweep writes the table alone -- never U, L or id.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "chs_look.h"
#include "chs_cc_host.h"

#define SH_THREADS 256
#define SH_WAVES (SH_THREADS / CHS_WAVE)
// LDS of a workgroup of the sweep: SH_SLOTS slots of CHS_SH_COLS 8-byte cells, cell 0 (`first` is not accumulated) being
// the slot's key.  256 slots are 32 KiB: five workgroups, 20 wavefronts, are resident on a CU's 160 KiB -- enough to hide
// the latency of the seven loads a pixel makes -- and a 64 x 64 tile of a phase-separated field holds a few dozen
// droplets, far fewer than 256.  (The 1024 slots of k_cc_stats would be 128 KiB: one workgroup per CU.)  A label whose slot
// is taken -- noise, a checkerboard -- spills to the table, which costs time and nothing else.
#define SH_SLOT_BITS 8
#define SH_SLOTS (1 << SH_SLOT_BITS)
#define SH_EMPTY (~0ull)
#define SH_SUM_BLOCKS 1024
#define SH_FIX 1073741824.0   // 2^CHS_CT_FIX_BITS
// the words of a look
#define SH_W_VIOL 0
#define SH_NW 2
// the words the table is reduced to on the device: the eight column sums, holes, inner_round
#define SH_NSUM 10

static_assert(CHS_CC_TC == CHS_WAVE && CHS_CC_TR % SH_WAVES == 0, "a wavefront sweeps whole tile rows");
static_assert(CHS_SH_WORDS == CHS_CC_WORDS + SH_NSUM, "the summary: the component words, then the reduced ones");
static_assert(CHS_CT_FIX_BITS == 30, "SH_FIX");

typedef unsigned long long sh_u64;
typedef long long sh_i64;
static_assert(sizeof(sh_i64) == sizeof(int64_t), "the table's cells");

struct ShSum { sh_i64 w[SH_NSUM]; };

// ---- 1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SH_THREADS) void k_sh_init(const int* __restrict__ cc_table, int C, sh_i64* __restrict__ table) {
  const int r = blockIdx.x * SH_THREADS + threadIdx.x;
  if (r >= C) return;
  sh_i64* row = table + (size_t)r * CHS_SH_COLS;
  row[CHS_SH_FIRST] = cc_table[(size_t)r * CHS_CC_COLS];
#pragma unroll
  for (int c = 1; c < CHS_SH_COLS; ++c) row[c] = 0;
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
// sum of n^2 over 0 <= n < m
__device__ __forceinline__ sh_i64 sh_squares_below(sh_i64 m) { return (m - 1) * m * (2 * m - 1) / 6; }

// cells[c] += v[c], c = 1 .. CHS_SH_COLS - 1, the zeros left out (most of a run's cells are zero)
template <typename P>
__device__ __forceinline__ void sh_add(P cells, const sh_i64 (&v)[CHS_SH_COLS]) {
#pragma unroll
  for (int c = 1; c < CHS_SH_COLS; ++c)
    if (v[c] != 0) atomicAdd(cells + c, (sh_u64)v[c]);
}

// grid (column tiles, row tiles).  No load is guarded by a branch: a pixel or a neighbour outside the grid is clamped to
// the pixel itself (or to the grid's last pixel) and masked.
template <typename T, bool NT>
__global__ __launch_bounds__(SH_THREADS) void k_sh_sweep(const void* Uv, const int* __restrict__ L, const int* __restrict__ id,
                                                         int N, int conn, int C, sh_u64* __restrict__ table, int* __restrict__ words) {
  __shared__ sh_u64 slot[SH_SLOTS * CHS_SH_COLS];
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = blockIdx.x * CHS_CC_TC + lane;
  for (int s = threadIdx.x; s < SH_SLOTS * CHS_SH_COLS; s += SH_THREADS) slot[s] = (s % CHS_SH_COLS) ? 0ull : SH_EMPTY;
  __syncthreads();
  const bool c8 = conn == 8;
  int viol = 0;
#pragma unroll 1
  for (int it = 0; it < CHS_CC_TR / SH_WAVES; ++it) {
    const int i = blockIdx.y * CHS_CC_TR + it * SH_WAVES + wave;
    const bool inb = i < N && j < N;
    const bool right = inb && j + 1 < N, down = inb && i + 1 < N, left = inb && j > 0;
    const int p = (i < N ? i : N - 1) * N + (j < N ? j : N - 1);
    const int l = inb ? L[p] : -2;
    T xs[1];
    chs_load<T, 1, NT>(U + p, xs);
    const int lr = L[right ? p + 1 : p], ld = L[down ? p + N : p], ll = L[left ? p - 1 : p];
    const int ldr = L[(down && right) ? p + N + 1 : p], ldl = L[(down && left) ? p + N - 1 : p];
    // the pixel a and its neighbours: b right, c below, d below right (the order of the definition), e below left, w left
    const bool a = l >= 0;
    const bool b = right && lr >= 0, c = down && ld >= 0, d = down && right && ldr >= 0;
    const bool e = down && left && ldl >= 0, w = left && ll >= 0;
    const double x = (double)xs[0];
    const bool inside = fabs(x) <= 4.0;   // (false for a NaN)
    sh_i64 fu = 0, fuu = 0;
    if (a && inside) { fu = (sh_i64)(x * SH_FIX); fuu = (sh_i64)((x * x) * SH_FIX); }
    // what the pixel adds to its own component
    const unsigned long long bPh = __ballot(a && b), bPv = __ballot(a && c);
    const unsigned long long bD1 = __ballot(c8 && a && d), bD2 = __ballot(c8 && a && e);
    // a cell of three: its first pixel is a (the cell below right of the pixel) or, with w background, the pixel is the
    // b of the cell below left of it
    const unsigned long long bT1 = __ballot(c8 && a && ((b ? 1 : 0) + (c ? 1 : 0) + (d ? 1 : 0)) == 2 && down && right);
    const unsigned long long bT2 = __ballot(c8 && a && left && !w && e && c);
    const unsigned long long bQ = __ballot(a && b && c && d);
    const unsigned long long bOut = __ballot(a && !inside);
    // the runs: every lane takes part in the cross-lane operations
    const int before = __shfl_up(l, 1, CHS_WAVE);
    const bool head = lane == 0 || before != l;
    const unsigned long long heads = __ballot(head);
    const unsigned long long rest = lane == CHS_WAVE - 1 ? 0ull : heads >> (lane + 1);
    const int len = rest ? __ffsll((long long)rest) : CHS_WAVE - lane;   // lanes from here to the run's end
    if (__ballot(a)) {   // (uniform) the segmented suffix sums: lane <- the sum over [lane, end of its run)
#pragma unroll
      for (int off = 1; off < CHS_WAVE; off <<= 1) {
        const sh_i64 u1 = __shfl_down(fu, off, CHS_WAVE), u2 = __shfl_down(fuu, off, CHS_WAVE);
        if (off < len) { fu += u1; fuu += u2; }
      }
    }
    if (head && a) {
      const unsigned long long m = (len == CHS_WAVE ? ~0ull : ((1ull << len) - 1ull)) << lane;
      const sh_i64 n = len, i64 = i, j0 = j;
      sh_i64 v[CHS_SH_COLS];
      v[CHS_SH_FIRST] = 0;
      v[CHS_SH_AREA] = n;
      v[CHS_SH_PAIRS_H] = __popcll(bPh & m);
      v[CHS_SH_PAIRS_V] = __popcll(bPv & m);
      v[CHS_SH_PAIRS_D] = __popcll(bD1 & m) + __popcll(bD2 & m);
      v[CHS_SH_TRIPLES] = __popcll(bT1 & m) + __popcll(bT2 & m);
      v[CHS_SH_QUADS] = __popcll(bQ & m);
      v[CHS_SH_WALL] = n * ((i == 0 ? 1 : 0) + (i == N - 1 ? 1 : 0)) + (j == 0 ? 1 : 0) + (j + len == N ? 1 : 0);
      v[CHS_SH_SI] = i64 * n;
      v[CHS_SH_SJ] = n * j0 + n * (n - 1) / 2;
      v[CHS_SH_SII] = i64 * i64 * n;
      v[CHS_SH_SJJ] = sh_squares_below(j0 + n) - sh_squares_below(j0);
      v[CHS_SH_SIJ] = i64 * v[CHS_SH_SJ];
      v[CHS_SH_SU_FIX] = fu;
      v[CHS_SH_SUU_FIX] = fuu;
      v[CHS_SH_N_OUTSIDE] = __popcll(bOut & m);
      const unsigned h = ((unsigned)l * 2654435761u) >> (32 - SH_SLOT_BITS);
      sh_u64* cells = slot + h * CHS_SH_COLS;
      const sh_u64 was = atomicCAS(cells, SH_EMPTY, (sh_u64)l);
      if (was == SH_EMPTY || was == (sh_u64)l) {
        sh_add(cells, v);
      } else {
        const int row = id[l];
        if ((unsigned)row < (unsigned)C) sh_add(table + (size_t)row * CHS_SH_COLS, v);
        else ++viol;   // (a label without a number: counted, never written)
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < SH_SLOTS; s += SH_THREADS) {
    const sh_u64 key = slot[s * CHS_SH_COLS];
    if (key == SH_EMPTY) continue;
    const int row = id[(int)key];
    if ((unsigned)row >= (unsigned)C) { ++viol; continue; }
    sh_u64* r = table + (size_t)row * CHS_SH_COLS;
#pragma unroll
    for (int c = 1; c < CHS_SH_COLS; ++c) {
      const sh_u64 x = slot[s * CHS_SH_COLS + c];
      if (x != 0) atomicAdd(r + c, x);
    }
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) viol += __shfl_down(viol, off, CHS_WAVE);
  if (lane == 0 && viol) atomicAdd(&words[SH_W_VIOL], viol);
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ ShSum sh_sum_of_row(const sh_i64* row, int conn) {
  const sh_i64 area = row[CHS_SH_AREA], ph = row[CHS_SH_PAIRS_H], pv = row[CHS_SH_PAIRS_V], pd = row[CHS_SH_PAIRS_D];
  const sh_i64 tr = row[CHS_SH_TRIPLES], q = row[CHS_SH_QUADS];
  const sh_i64 euler = conn == 8 ? area - ph - pv - pd + tr + 3 * q : area - ph - pv + q;
  ShSum s;
  s.w[0] = area; s.w[1] = ph; s.w[2] = pv; s.w[3] = pd; s.w[4] = tr; s.w[5] = q;
  s.w[6] = row[CHS_SH_WALL]; s.w[7] = row[CHS_SH_N_OUTSIDE];
  s.w[8] = 1 - euler;
  s.w[9] = row[CHS_SH_WALL] == 0 ? 1 : 0;
  return s;
}

__device__ __forceinline__ ShSum sh_sum_add(const ShSum& x, const ShSum& y) {
  ShSum s;
#pragma unroll
  for (int k = 0; k < SH_NSUM; ++k) s.w[k] = x.w[k] + y.w[k];
  return s;
}

__device__ __forceinline__ ShSum sh_block_sum(ShSum mine, ShSum* red) {
  red[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int off = SH_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = sh_sum_add(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

// part[block] <- the sums of the rows block, block + gridDim.x, ... (a thread adds its rows in ascending order)
__global__ __launch_bounds__(SH_THREADS) void k_sh_summary_rows(const sh_i64* __restrict__ table, int C, int conn, ShSum* __restrict__ part) {
  __shared__ ShSum red[SH_THREADS];
  ShSum s = {};
  for (int r = blockIdx.x * SH_THREADS + threadIdx.x; r < C; r += gridDim.x * SH_THREADS)
    s = sh_sum_add(s, sh_sum_of_row(table + (size_t)r * CHS_SH_COLS, conn));
  s = sh_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(SH_THREADS) void k_sh_summary_fin(const ShSum* __restrict__ part, int nparts, ShSum* __restrict__ out) {
  __shared__ ShSum red[SH_THREADS];
  ShSum s = {};
  for (int r = threadIdx.x; r < nparts; r += SH_THREADS) s = sh_sum_add(s, part[r]);
  s = sh_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct ShResult {   // pinned
  int words[SH_NW];
  ShSum out;
};

struct ShBuf : LookBase {   // have: table and count are the look's snapshot
  sh_i64* table = nullptr;   // [cap][CHS_SH_COLS]
  sh_i64 cap = 0;
  int* words = nullptr;      // [SH_NW]
  ShSum* part = nullptr;     // [SH_SUM_BLOCKS]
  ShSum* out = nullptr;      // [1]
  ShResult* hRes = nullptr;
  sh_i64 count = 0;
};

void sh_release(ShBuf* s) {
  if (!s) return;
  hipFree(s->table); hipFree(s->words); hipFree(s->part); hipFree(s->out);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int sh_alloc(ShBuf* s) {
  CHS_HIP(hipMalloc(&s->words, sizeof(int) * SH_NW));
  CHS_HIP(hipMalloc(&s->part, sizeof(ShSum) * SH_SUM_BLOCKS));
  CHS_HIP(hipMalloc(&s->out, sizeof(ShSum)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(ShResult), hipHostMallocDefault));
  return CHS_OK;
}

template <typename T>
int launch_sweep(const ShBuf* s, const void* U, const ChsCcSnapshot& cc, int conn, hipStream_t st) {
  const int N = s->N;
  const dim3 grid(chs_cc::tiles_of(N, CHS_CC_TC), chs_cc::tiles_of(N, CHS_CC_TR));
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  if (chs_grid_exceeds_cache((size_t)N, sizeof(T)))
    k_sh_sweep<T, true><<<grid, SH_THREADS, 0, st>>>(U, cc.L, cc.id, N, conn, (int)cc.count, (sh_u64*)s->table, s->words);
  else
    k_sh_sweep<T, false><<<grid, SH_THREADS, 0, st>>>(U, cc.L, cc.id, N, conn, (int)cc.count, (sh_u64*)s->table, s->words);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// The sweep and the summary behind a components look that has just succeeded on `cc`.
int sh_run(ShBuf* s, Engine* E, hipStream_t st, const ChsCcSnapshot& cc, int conn, const int64_t* ccw, const std::string& who) {
  const sh_i64 C = cc.count;
  look_forget(s);
  if (C > s->cap) {   // the table grows with the component table
    CHS_HIP(hipFree(s->table));
    s->table = nullptr; s->cap = 0;
    const sh_i64 cap = C + C / 8 + 1024;
    CHS_HIP(hipMalloc(&s->table, sizeof(sh_i64) * CHS_SH_COLS * (size_t)cap));
    s->cap = cap;
  }
  CHS_HIP(hipMemsetAsync(s->words, 0, sizeof(int) * SH_NW, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  if (C > 0) {
    k_sh_init<<<(int)((C + SH_THREADS - 1) / SH_THREADS), SH_THREADS, 0, st>>>(cc.table, (int)C, s->table);
    CHS_HIP(hipGetLastError());
    const int rc = E->dtype == CHS_F64 ? launch_sweep<double>(s, E->dU, cc, conn, st) : launch_sweep<float>(s, E->dU, cc, conn, st);
    if (rc) return rc;
  }
  const int parts = C > 0 ? (int)std::min<sh_i64>((C + SH_THREADS - 1) / SH_THREADS, SH_SUM_BLOCKS) : 1;
  k_sh_summary_rows<<<parts, SH_THREADS, 0, st>>>(s->table, (int)C, conn, s->part);
  CHS_HIP(hipGetLastError());
  k_sh_summary_fin<<<1, SH_THREADS, 0, st>>>(s->part, parts, s->out);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * SH_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(ShSum), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  if (s->hRes->words[SH_W_VIOL]) {
    chs_set_error(who + ": self-check failed: " + std::to_string(s->hRes->words[SH_W_VIOL]) + " labels without a component number");
    return CHS_ECHECK;
  }
  if (s->hRes->out.w[0] != ccw[CHS_CC_AREA]) {
    chs_set_error(who + ": self-check failed: the areas of the table add up to " + std::to_string(s->hRes->out.w[0]) +
                  ", the components look counted " + std::to_string(ccw[CHS_CC_AREA]));
    return CHS_ECHECK;
  }
  s->count = C;
  return look_end(s);
}
}  // namespace

void chs_sh_free(void** buf) {
  if (!buf) return;
  sh_release((ShBuf*)*buf);
  *buf = nullptr;
}

void chs_sh_forget(void* buf) {
  if (!buf) return;
  ShBuf* s = (ShBuf*)buf;
  look_forget(s);
  s->count = 0;
}

int chs_sh_look(Engine* E, hipStream_t st, void** ccbuf, void** buf, double threshold, int32_t connectivity, int32_t side,
                int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  int64_t ccw[CHS_CC_WORDS];
  // the components look: its own checks of connectivity, side and field, in its own order, under this look's name
  if ((rc = chs_cc_look(E, st, ccbuf, threshold, connectivity, side, ccw, who_))) return rc;
  if ((rc = look_buffers<ShBuf>(buf, E->N, sh_alloc, sh_release))) return rc;
  ShBuf* s = (ShBuf*)*buf;
  ChsCcSnapshot cc;
  if ((rc = chs_cc_snapshot(*ccbuf, &cc, who_))) return rc;
  if ((rc = sh_run(s, E, st, cc, connectivity, ccw, who))) return rc;
  memcpy(out, ccw, sizeof(int64_t) * CHS_CC_WORDS);
  memcpy(out + CHS_CC_WORDS, s->hRes->out.w, sizeof(int64_t) * SH_NSUM);
  return CHS_OK;
}

int chs_sh_table(void* buf, int device, hipStream_t st, int64_t rows, int64_t* out, const char* who_) {
  const std::string who(who_);
  const ShBuf* s = (const ShBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (rows != s->count) { chs_set_error(who + ": rows = " + std::to_string(rows) + ", the last look counted " + std::to_string(s->count)); return CHS_EINVAL; }
  if (rows == 0) return CHS_OK;
  return look_fetch(device, st, out, s->table, sizeof(int64_t) * CHS_SH_COLS * (size_t)rows);
}

int chs_sh_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const ShBuf*)buf, ms, what);
}

extern "C" int chs_shapes(chs_handle h, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_SH_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_shapes: null handle"); return CHS_EINVAL; }
  return chs_sh_look(E, E->stream, &E->cc, &E->sh, threshold, connectivity, side, out, "chs_shapes");
}

extern "C" int chs_shapes_table(chs_handle h, int64_t rows, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_shapes_table: null handle"); return CHS_EINVAL; }
  return chs_sh_table(E->sh, E->hc.device, E->stream, rows, out, "chs_shapes_table");
}

extern "C" int chs_shapes_last_ms(chs_handle h, double* ms) {
  return chs_sh_last_ms(h, h ? ((Engine*)h)->sh : nullptr, ms, "chs_shapes");
}
