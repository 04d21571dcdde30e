// chs_track.hip -- droplet tracking on the device: the labelling of now overlapped with the labelling of an earlier look,
// one int64 row (a, b, n) per pair of component numbers that share pixels (the definition:
// include/chs_hip.h, chs_track).
//
// A track look is a shapes look first: chs_sh_look labels the field and fills the shape table, and leaves the root label
// of every pixel (L) and the number at every root (id) on the component buffers.  Then, here:
//   1  k_tr_heads    one sweep over L, id and the frame (the number image an earlier track look kept): writes the number
//                    image of now, id[L[p]] or -1, and counts the heads -- the pixels with a key other than (-1, -1) whose
//                    key differs from the left and from the upper neighbour's.  The raster-first pixel of every key is a
//                    head, so the number of keys P is at most HEADS; the host reads HEADS and sizes the hash table to the
//                    power of two >= 2 HEADS: the load never passes 1/2 and no insert can fail to find a free slot.
//   2  k_tr_sweep    one sweep over the two number images.  A workgroup per CHS_CC_TR x CHS_CC_TC tile, a wavefront per tile
//                    row, a lane per pixel.  A run of equal keys inside the wavefront's row is ONE contribution, its length,
//                    made by the run's first lane.  It goes to an LDS slot (64-bit key taken by compare-and-swap, 64-bit
//                    count) where the slot is free or holds that key, and straight to the global table otherwise; the LDS
//                    slots are added to the global table at the end.  The global table: open addressing, linear probing,
//                    the key word claimed by a 64-bit compare-and-swap from 0, the count added by a 64-bit atomic add; a
//                    device counter counts the claims, which is P.
//   3  k_tr_compact  the occupied slots to a row list; the host sorts the P rows by key.
// Every cell is an integer and every accumulation an integer add: the table does not depend on the order of the atomics.
// No loop of a kernel waits for another thread: every probe loop is bounded by the slot count and raises a flag at its end.
// The kernels read int32 images only -- never the field.
#include <algorithm>
#include <cstring>
#include <vector>

#include "chs_look.h"
#include "chs_cc_host.h"

#define TR_THREADS 256
#define TR_WAVES (TR_THREADS / CHS_WAVE)
// LDS of a workgroup of the sweep: TR_SLOTS slots of a 64-bit key and a 64-bit count.  1024 slots are 16 KiB: the eight
// workgroups (32 wavefronts) a CU can hold by its wavefront limit fit into its 160 KiB, so LDS does not bound the
// occupancy, and a 64 x 64 tile of a phase-separated field holds a few dozen droplets and so at most a few hundred keys:
// every one finds its slot.  (2048 slots would be 32 KiB: five workgroups per CU, for keys that only noise has.)  A key
// whose slot is taken -- noise, stripes against stripes -- goes to the global table, which costs time and nothing else.
#define TR_SLOT_BITS 10
#define TR_SLOTS (1 << TR_SLOT_BITS)
#define TR_MIN_SLOTS 1024ull
#define TR_HEAD_BLOCKS 2048   // workgroups of k_tr_heads at most: eight a CU
// The global table may take this many bytes (16 per slot): 2 GiB, 2^27 slots, up to 2^26 heads.  Noise at N = 8192 has
// ~N^2 / 2 = 2^25 heads and fits; a droplet field has a number of heads of the order of its interface length.
#define TR_MAX_TABLE_BYTES (2ull << 30)
// the device words of a look
#define TR_W_HEADS 0
#define TR_W_BG 1       // pixels with the key (-1, -1)
#define TR_W_CLAIMS 2   // key words claimed in the global table: P
#define TR_W_ROWS 3     // rows k_tr_compact wrote
#define TR_W_FLAG 4     // a probe loop reached its end, or a row beyond the row list
#define TR_W_VIOL 5     // labels without a component number
#define TR_NW 8

static_assert(CHS_CC_TC == CHS_WAVE && CHS_CC_TR % TR_WAVES == 0, "a wavefront sweeps whole tile rows");
static_assert(CHS_TR_WORDS == CHS_SH_WORDS + 8, "the words: those of the shapes look, then the overlap's");

typedef unsigned long long tr_u64;
typedef long long tr_i64;
static_assert(sizeof(tr_i64) == sizeof(int64_t), "the table's cells");

// the key of a pixel: never 0 for a counted one
__device__ __forceinline__ tr_u64 tr_key(int a, int b) { return ((tr_u64)(unsigned)(a + 1) << 32) | (tr_u64)(unsigned)(b + 1); }
// the upper `bits` bits of a multiplicative hash of the whole key (a and b alone or xor-ed would put every continued
// droplet, a == b, into neighbouring or equal slots)
__device__ __forceinline__ unsigned tr_hash(tr_u64 key, int bits) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits)); }

// ---- 1 ---------------------------------------------------------------------------------------------------------------
// a thread per pixel, a workgroup striding over the grid: the launch has at most TR_HEAD_BLOCKS workgroups, so that the
// three counters take a few thousand atomic adds and not one per 256 pixels.  frame == nullptr: no frame, every a is -1
// (the look only writes the number image).
__global__ __launch_bounds__(TR_THREADS) void k_tr_heads(const int* __restrict__ L, const int* __restrict__ id,
                                                         const int* __restrict__ frame, int* __restrict__ now, int N, int n2,
                                                         int C, tr_u64* __restrict__ words) {
  __shared__ int cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  int nh = 0, nb = 0, nv = 0;
  for (int base = blockIdx.x * TR_THREADS; base < n2; base += gridDim.x * TR_THREADS) {
    const int p = base + threadIdx.x;
    if (p >= n2) continue;
    const int i = p / N, j = p - i * N;
    const int l = L[p];
    int b = -1;
    if (l >= 0) {
      b = id[l];
      if ((unsigned)b >= (unsigned)C) { ++nv; b = -1; }   // (counted, never used as a number)
    }
    now[p] = b;
    const int a = frame ? frame[p] : -1;
    const bool left = j > 0, up = i > 0;
    const int ll = L[left ? p - 1 : p], lu = L[up ? p - N : p];
    const int al = (frame && left) ? frame[p - 1] : a, au = (frame && up) ? frame[p - N] : a;
    const bool bg = a < 0 && l < 0;
    if (bg) ++nb;
    else if ((!left || ll != l || al != a) && (!up || lu != l || au != a)) ++nh;
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) {
    nh += __shfl_down(nh, off, CHS_WAVE);
    nb += __shfl_down(nb, off, CHS_WAVE);
    nv += __shfl_down(nv, off, CHS_WAVE);
  }
  if ((threadIdx.x & (CHS_WAVE - 1)) == 0) {
    if (nh) atomicAdd(&cnt[0], nh);
    if (nb) atomicAdd(&cnt[1], nb);
    if (nv) atomicAdd(&cnt[2], nv);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (cnt[0]) atomicAdd(&words[TR_W_HEADS], (tr_u64)cnt[0]);
    if (cnt[1]) atomicAdd(&words[TR_W_BG], (tr_u64)cnt[1]);
    if (cnt[2]) atomicAdd(&words[TR_W_VIOL], (tr_u64)cnt[2]);
  }
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
// table[slot] = (key, count).  n pixels of `key` into the global table; false: no slot in `slots` probes.
__device__ __forceinline__ bool tr_insert(tr_u64* __restrict__ table, int bits, tr_u64 key, tr_u64 n, tr_u64* __restrict__ words) {
  const tr_u64 slots = 1ull << bits, mask = slots - 1ull;
  tr_u64 s = tr_hash(key, bits);
  for (tr_u64 probe = 0; probe < slots; ++probe) {
    tr_u64* cell = table + 2ull * s;
    const tr_u64 was = atomicCAS(cell, 0ull, key);
    if (was == 0ull) atomicAdd(&words[TR_W_CLAIMS], 1ull);
    if (was == 0ull || was == key) {
      atomicAdd(cell + 1, n);
      return true;
    }
    s = (s + 1ull) & mask;
  }
  return false;
}

// grid (column tiles, row tiles).  No load is guarded by a branch: a pixel outside the grid is clamped to the grid's last
// pixel and masked.
__global__ __launch_bounds__(TR_THREADS) void k_tr_sweep(const int* __restrict__ frame, const int* __restrict__ now, int N,
                                                         tr_u64* __restrict__ table, int bits, tr_u64* __restrict__ words) {
  __shared__ tr_u64 slot[2 * TR_SLOTS];
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = blockIdx.x * CHS_CC_TC + lane;
  for (int s = threadIdx.x; s < 2 * TR_SLOTS; s += TR_THREADS) slot[s] = 0ull;
  __syncthreads();
  int fail = 0;
#pragma unroll 1
  for (int it = 0; it < CHS_CC_TR / TR_WAVES; ++it) {
    const int i = blockIdx.y * CHS_CC_TR + it * TR_WAVES + wave;
    const bool inb = i < N && j < N;
    const int p = (i < N ? i : N - 1) * N + (j < N ? j : N - 1);
    const int a = frame[p], b = now[p];
    const tr_u64 key = (inb && (a >= 0 || b >= 0)) ? tr_key(a, b) : 0ull;
    // the runs: every lane takes part in the cross-lane operations
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const unsigned bhi = __shfl_up(hi, 1, CHS_WAVE), blo = __shfl_up(lo, 1, CHS_WAVE);
    const bool head = lane == 0 || bhi != hi || blo != lo;
    const unsigned long long heads = __ballot(head);
    const unsigned long long rest = lane == CHS_WAVE - 1 ? 0ull : heads >> (lane + 1);
    const int len = rest ? __ffsll((long long)rest) : CHS_WAVE - lane;   // lanes from here to the run's end
    if (head && key != 0ull) {
      tr_u64* cell = slot + 2u * tr_hash(key, TR_SLOT_BITS);
      const tr_u64 was = atomicCAS(cell, 0ull, key);
      if (was == 0ull || was == key) atomicAdd(cell + 1, (tr_u64)len);
      else if (!tr_insert(table, bits, key, (tr_u64)len, words)) ++fail;
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < TR_SLOTS; s += TR_THREADS) {
    const tr_u64 key = slot[2 * s];
    if (key == 0ull) continue;
    if (!tr_insert(table, bits, key, slot[2 * s + 1], words)) ++fail;
  }
  if (fail) atomicAdd(&words[TR_W_FLAG], (tr_u64)fail);
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
// a thread per slot: rows[r] = (a, b, n) in the order the atomics fell (the host sorts)
__global__ __launch_bounds__(TR_THREADS) void k_tr_compact(const tr_u64* __restrict__ table, tr_u64 slots, tr_i64* __restrict__ rows,
                                                           tr_u64 cap, tr_u64* __restrict__ words) {
  const tr_u64 s = (tr_u64)blockIdx.x * TR_THREADS + threadIdx.x;
  if (s >= slots) return;
  const tr_u64 key = table[2ull * s];
  if (key == 0ull) return;
  const tr_u64 r = atomicAdd(&words[TR_W_ROWS], 1ull);
  if (r >= cap) { atomicAdd(&words[TR_W_FLAG], 1ull); return; }
  rows[3ull * r] = (tr_i64)(key >> 32) - 1;
  rows[3ull * r + 1] = (tr_i64)(key & 0xffffffffull) - 1;
  rows[3ull * r + 2] = (tr_i64)table[2ull * s + 1];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct TrRow { int64_t a, b, n; };
static_assert(sizeof(TrRow) == 3 * sizeof(int64_t), "a row of the pair table");

// One structure for both halves of a track look: the frame (per handle; per member in a batch) and the working set --
// words, hash table, row list, the sorted rows of the last look (per handle; one for a batch).  A single handle uses one
// TrBuf for both; what a half does not use is never allocated.
struct TrBuf : LookBase {   // have: `rows` is the last look's pair table
  // the frame
  int* img[2] = {nullptr, nullptr};   // [N * N] number images: img[cur] is the frame, img[cur ^ 1] the one a look writes
  int cur = 0;
  bool haveFrame = false;
  int64_t frameCount = 0, frameArea = 0;
  double frameThreshold = 0.0;
  int frameConn = 0, frameSide = 0;
  // the working set
  tr_u64* words = nullptr;     // [TR_NW]
  tr_u64* hWords = nullptr;    // pinned
  tr_u64* table = nullptr;     // [slotsCap][2]
  tr_u64 slotsCap = 0;
  tr_i64* drows = nullptr;     // [rowsCap][3]
  tr_u64 rowsCap = 0;
  hipEvent_t evMid[2] = {nullptr, nullptr};   // behind k_tr_heads, in front of the sweep: the host's wait between them is not device time
  std::vector<TrRow> rows;     // sorted by (a, b)
};

void tr_release(TrBuf* s) {
  if (!s) return;
  hipFree(s->img[0]); hipFree(s->img[1]); hipFree(s->words); hipFree(s->table); hipFree(s->drows);
  if (s->hWords) hipHostFree(s->hWords);
  for (auto e : s->evMid) if (e) hipEventDestroy(e);
  look_release_events(s);
  delete s;
}

int tr_alloc(TrBuf*) { return CHS_OK; }   // (each half at its first use: tr_frame_ready, tr_work_ready)

int tr_frame_ready(TrBuf* f) {
  const size_t n2 = (size_t)f->N * f->N;
  for (auto& im : f->img)
    if (!im) CHS_HIP(hipMalloc(&im, sizeof(int) * n2));
  return CHS_OK;
}

int tr_work_ready(TrBuf* w) {
  if (!w->words) CHS_HIP(hipMalloc(&w->words, sizeof(tr_u64) * TR_NW));
  if (!w->hWords) CHS_HIP(hipHostMalloc((void**)&w->hWords, sizeof(tr_u64) * TR_NW, hipHostMallocDefault));
  for (auto& e : w->evMid)
    if (!e) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

void tr_drop_frame(TrBuf* f) {
  f->haveFrame = false;
  f->frameCount = f->frameArea = 0;
}

// The overlap behind a shapes look that has just succeeded on `cc`: f holds the frame, w the working set.
int tr_run(TrBuf* f, TrBuf* w, hipStream_t st, const ChsCcSnapshot& cc, const int64_t* shw, double threshold, int conn, int side,
           int keep, int64_t* out, const std::string& who) {
  const int N = f->N, n2 = N * N;
  const tr_i64 C = cc.count;
  int rc;
  look_forget(w);
  w->rows.clear();
  if ((rc = tr_work_ready(w))) return rc;
  const bool prev = f->haveFrame;
  int64_t ow[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // HAVE_PREV, PREV_COUNT, PAIRS, OVERLAP, LOST, GAINED, HEADS, SLOTS
  if (prev || keep) {
    if ((rc = tr_frame_ready(f))) return rc;
  }
  int* now = f->img[f->cur ^ 1];
  CHS_HIP(hipMemsetAsync(w->words, 0, sizeof(tr_u64) * TR_NW, st));
  CHS_HIP(hipEventRecord(w->ev[0], st));
  if (prev || keep) {
    k_tr_heads<<<std::min((n2 + TR_THREADS - 1) / TR_THREADS, TR_HEAD_BLOCKS), TR_THREADS, 0, st>>>(cc.L, cc.id, prev ? f->img[f->cur] : nullptr, now, N, n2,
                                                                         (int)C, w->words);
    CHS_HIP(hipGetLastError());
  }
  CHS_HIP(hipEventRecord(w->evMid[0], st));
  if (prev) {
    CHS_HIP(hipMemcpyAsync(w->hWords, w->words, sizeof(tr_u64) * TR_NW, hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    const tr_u64 heads = w->hWords[TR_W_HEADS];
    tr_u64 slots = TR_MIN_SLOTS;
    int bits = 10;
    while (slots < 2ull * heads) { slots <<= 1; ++bits; }
    if (slots * 16ull > TR_MAX_TABLE_BYTES) {
      chs_set_error(who + ": " + std::to_string(heads) + " heads need a hash table of " + std::to_string(slots * 16ull) +
                    " bytes, above the cap of " + std::to_string(TR_MAX_TABLE_BYTES));
      return CHS_EHIP;   // (the code of an allocation the device refuses)
    }
    if (slots > w->slotsCap) {
      CHS_HIP(hipFree(w->table));
      w->table = nullptr; w->slotsCap = 0;
      CHS_HIP(hipMalloc(&w->table, 16ull * slots));
      w->slotsCap = slots;
    }
    const tr_u64 needRows = heads > 0 ? heads : 1;
    if (needRows > w->rowsCap) {
      CHS_HIP(hipFree(w->drows));
      w->drows = nullptr; w->rowsCap = 0;
      const tr_u64 cap = needRows + needRows / 8 + 1024;
      CHS_HIP(hipMalloc(&w->drows, sizeof(tr_i64) * 3 * cap));
      w->rowsCap = cap;
    }
    CHS_HIP(hipMemsetAsync(w->table, 0, 16ull * slots, st));
    CHS_HIP(hipEventRecord(w->evMid[1], st));
    const dim3 grid(chs_cc::tiles_of(N, CHS_CC_TC), chs_cc::tiles_of(N, CHS_CC_TR));
    k_tr_sweep<<<grid, TR_THREADS, 0, st>>>(f->img[f->cur], now, N, w->table, bits, w->words);
    CHS_HIP(hipGetLastError());
    k_tr_compact<<<(unsigned)((slots + TR_THREADS - 1) / TR_THREADS), TR_THREADS, 0, st>>>(w->table, slots, w->drows, heads, w->words);
    CHS_HIP(hipGetLastError());
    CHS_HIP(hipEventRecord(w->ev[1], st));
    CHS_HIP(hipMemcpyAsync(w->hWords, w->words, sizeof(tr_u64) * TR_NW, hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    const tr_u64* hw = w->hWords;
    if (hw[TR_W_VIOL]) {
      chs_set_error(who + ": self-check failed: " + std::to_string(hw[TR_W_VIOL]) + " labels without a component number");
      return CHS_ECHECK;
    }
    if (hw[TR_W_FLAG] || hw[TR_W_CLAIMS] > heads || hw[TR_W_ROWS] != hw[TR_W_CLAIMS]) {
      chs_set_error(who + ": self-check failed: " + std::to_string(hw[TR_W_FLAG]) + " inserts without a slot, " +
                    std::to_string(hw[TR_W_CLAIMS]) + " keys, " + std::to_string(hw[TR_W_ROWS]) + " rows, " + std::to_string(heads) + " heads");
      return CHS_ECHECK;
    }
    const tr_u64 P = hw[TR_W_CLAIMS];
    const tr_u64 bg = hw[TR_W_BG];
    w->rows.resize((size_t)P);
    if (P > 0) {
      CHS_HIP(hipMemcpyAsync(w->rows.data(), w->drows, sizeof(TrRow) * (size_t)P, hipMemcpyDeviceToHost, st));
      CHS_HIP(hipStreamSynchronize(st));
    }
    std::sort(w->rows.begin(), w->rows.end(), [](const TrRow& x, const TrRow& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    int64_t overlap = 0, lost = 0, gained = 0;
    for (const TrRow& r : w->rows) {
      if (r.a >= 0 && r.b >= 0) overlap += r.n;
      else if (r.a >= 0) lost += r.n;
      else gained += r.n;
    }
    if (overlap + lost + gained + (int64_t)bg != (int64_t)n2 || overlap + lost != f->frameArea || overlap + gained != shw[CHS_CC_AREA]) {
      w->rows.clear();
      chs_set_error(who + ": self-check failed: overlap " + std::to_string(overlap) + ", lost " + std::to_string(lost) + ", gained " +
                    std::to_string(gained) + ", background " + std::to_string(bg) + " of " + std::to_string(n2) + " pixels; the frame's area " +
                    std::to_string(f->frameArea) + ", the look's " + std::to_string(shw[CHS_CC_AREA]));
      return CHS_ECHECK;
    }
    ow[0] = 1; ow[1] = f->frameCount; ow[2] = (int64_t)P; ow[3] = overlap; ow[4] = lost; ow[5] = gained;
    ow[6] = (int64_t)heads; ow[7] = (int64_t)slots;
  } else {
    CHS_HIP(hipEventRecord(w->evMid[1], st));
    CHS_HIP(hipEventRecord(w->ev[1], st));
    CHS_HIP(hipMemcpyAsync(w->hWords, w->words, sizeof(tr_u64) * TR_NW, hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    if (w->hWords[TR_W_VIOL]) {
      chs_set_error(who + ": self-check failed: " + std::to_string(w->hWords[TR_W_VIOL]) + " labels without a component number");
      return CHS_ECHECK;
    }
  }
  if (keep) {   // the image of now becomes the frame: the two are swapped, nothing is copied
    f->cur ^= 1;
    f->haveFrame = true;
    f->frameCount = C; f->frameArea = shw[CHS_CC_AREA];
    f->frameThreshold = threshold; f->frameConn = conn; f->frameSide = side;
  }
  if ((rc = look_end(w))) return rc;
  float m0 = 0.f, m1 = 0.f;   // the overlap passes alone: without the host's wait for HEADS between them
  CHS_HIP(hipEventElapsedTime(&m0, w->ev[0], w->evMid[0]));
  CHS_HIP(hipEventElapsedTime(&m1, w->evMid[1], w->ev[1]));
  w->ms = (double)m0 + (double)m1;
  memcpy(out, shw, sizeof(int64_t) * CHS_SH_WORDS);
  memcpy(out + CHS_SH_WORDS, ow, sizeof ow);
  return CHS_OK;
}
}  // namespace

void chs_tr_free(void** buf) {
  if (!buf) return;
  tr_release((TrBuf*)*buf);
  *buf = nullptr;
}

void chs_tr_forget(void* buf) {
  if (!buf) return;
  TrBuf* s = (TrBuf*)buf;
  look_forget(s);
  s->rows.clear();
  tr_drop_frame(s);
}

void chs_tr_reset(void* frame) {
  if (frame) tr_drop_frame((TrBuf*)frame);
}

int chs_tr_look(Engine* E, hipStream_t st, void** ccbuf, void** shbuf, void** frame, void** work, double threshold,
                int32_t connectivity, int32_t side, int32_t keep, int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  int64_t shw[CHS_SH_WORDS];
  // the shapes look: its own checks (and those of the components look), in their own order, under this look's name
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if ((rc = chs_sh_look(E, st, ccbuf, shbuf, threshold, connectivity, side, shw, who_))) return rc;
  if ((rc = look_buffers<TrBuf>(frame, E->N, tr_alloc, tr_release))) return rc;
  if (work != frame && (rc = look_buffers<TrBuf>(work, E->N, tr_alloc, tr_release))) return rc;
  ChsCcSnapshot cc;
  if ((rc = chs_cc_snapshot(*ccbuf, &cc, who_))) return rc;
  return tr_run((TrBuf*)*frame, (TrBuf*)*work, st, cc, shw, threshold, connectivity, side, keep, out, who);
}

int chs_tr_pairs(void* work, int64_t rows, int64_t* out, const char* who_) {
  const std::string who(who_);
  const TrBuf* w = (const TrBuf*)work;
  int rc;
  if ((rc = look_ready(w, out, who))) return rc;
  if (rows != (int64_t)w->rows.size()) {
    chs_set_error(who + ": rows = " + std::to_string(rows) + ", the last look counted " + std::to_string(w->rows.size()));
    return CHS_EINVAL;
  }
  if (rows > 0) memcpy(out, w->rows.data(), sizeof(TrRow) * (size_t)rows);
  return CHS_OK;
}

extern "C" int chs_track(chs_handle h, double threshold, int32_t connectivity, int32_t side, int32_t keep, int64_t out[CHS_TR_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_track: null handle"); return CHS_EINVAL; }
  return chs_tr_look(E, E->stream, &E->cc, &E->sh, &E->tr, &E->tr, threshold, connectivity, side, keep, out, "chs_track");
}

extern "C" int chs_track_pairs(chs_handle h, int64_t rows, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_track_pairs: null handle"); return CHS_EINVAL; }
  return chs_tr_pairs(E->tr, rows, out, "chs_track_pairs");
}

extern "C" int chs_track_reset(chs_handle h) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_track_reset: null handle"); return CHS_EINVAL; }
  chs_tr_reset(E->tr);
  return CHS_OK;
}

extern "C" int chs_track_last_ms(chs_handle h, double* ms) {
  return look_last_ms(h, h ? (const TrBuf*)((Engine*)h)->tr : nullptr, ms, "chs_track");
}
