// chs_chords.hip -- chord lengths (linear intercepts) of both phases of the thresholded field on the device, along rows
// and along columns (the definition: include/chs_hip.h, chs_chords).
//
// Phases that depend on each other are separate launches: no workgroup ever waits for another one, nothing is polled.
//   1  k_ch_mask   one sweep over U gives both bit planes.  A workgroup thresholds one band of CHS_CH_WORD rows of a
//                  strip of CH_THREADS columns; a thread owns one column (the element loads: a wavefront's load is then
//                  CHS_CH_WORD consecutive pixels of a row, no load guarded by a branch).  Bit r of a thread's word is
//                  row r of the band of its column: the column plane, as k_dt_mask has it.  In the same iteration the
//                  ballot of the wavefront is the word of row r over the wavefront's 64 columns: the row plane for free;
//                  lane r keeps it, and after the band lane r stores the word of row r -- a coalesced store.  With
//                  16-byte loads a lane would own 2 or 4 neighbouring columns and the ballots of its elements would
//                  interleave; the element path needs no de-interleaving, at any N.
//                  Both planes are [nb][N] words, word index major, line minor: plane[k][l] holds pixels 64 k .. 64 k + 63
//                  of line l.  A bit is set where the pixel is phase 0; rows and columns outside the grid are clamped
//                  for the load and masked (their bits stay 0 and the walk never looks at them).
//   2  k_ch_walk   a thread owns one word of one line of one direction, and a chord is counted by the thread in whose word
//                  it ENDS.  Inside the word the runs are the trailing zeros of the word XORed with the run's phase; the
//                  bits beyond N of the last word are cut off by the count, not looked at.  The run that reaches the
//                  word's end is this word's only if the next word begins with the other phase (or the line ends).  The
//                  run of the word's first pixel began earlier: if it ends here the thread searches backwards, a whole
//                  word of the phase being 64 pixels more and the first other word ending the search by its leading
//                  zeros -- CH_BACK words loaded before they are looked at, the first CH_BACK with the word itself.  A
//                  word in the middle of a long chord does nothing, so all searches together read no more than every
//                  word once and one word per chord.  Two launch dimensions more than a thread per line: N^2 / 32
//                  threads, not 2 N, and no state carried along the line.
//                  A finished chord is one integer add: inner chords of length 1 and 2 -- almost all of a noise field --
//                  into four 16-bit counters packed in a register of the lane, summed over the wavefront by shuffles,
//                  the others into the workgroup's LDS histogram (lengths below CH_LBINS) or straight to the int64
//                  global one.  The LDS histogram is flushed by atomicAdd: integer sums, order-free.  Both loops have a
//                  cap they cannot reach; reaching it all the same sets a bit of the error word.
//   3  k_ch_fin    one workgroup reduces the eight histograms to the 24 words by a fixed tree and checks the look: per
//                  direction the chords add up to N^2 pixels, and the cut chords of both phases are N to 2 N.
// Nothing of the handle is written and nothing the step loop owns is read: its field alone.
#include <cstring>

#include "chs_look.h"
#include "chs_cc_host.h"   // chs_cc::fg_of: phase 0 is the foreground of chs_components with CHS_CC_BELOW

#define CHS_CH_WORD 64                      // pixels of a line in one word; rows of a band of k_ch_mask
#define CH_THREADS 256                      // k_ch_mask
#define CH_GROUP 256                        // lines of a workgroup of k_ch_walk
#define CH_LBINS 512                        // lengths below it go to the workgroup's LDS histogram
#define CH_BACK 4                           // words of a search backwards in flight
#define CH_FIN_THREADS 1024                 // k_ch_fin: one workgroup
#define CH_MAX_N 16384                      // N of chs_create at most: nb = 256 words a line, a grid dimension
#define CH_HISTS 8                          // phase, direction, class
// the words of a look
#define CH_W_ERR 0
#define CH_NW 2
#define CH_ERR_WALK 1                       // a loop of k_ch_walk (the runs of a word, the search backwards) reached its cap
#define CH_ERR_SUM 2                        // the chords of a direction do not add up to N^2 pixels
#define CH_ERR_CUT 4                        // the cut chords of a direction are not N .. 2 N

static_assert(CHS_CH_WORD == 64 && CHS_CH_WORD == CHS_WAVE, "a word is the ballot of one wavefront");
static_assert(CH_THREADS % CHS_WAVE == 0 && CH_GROUP % CHS_WAVE == 0, "whole wavefronts");
static_assert(CH_FIN_THREADS % (CH_HISTS * CHS_WAVE) == 0 && CH_FIN_THREADS <= 1024, "whole wavefronts per histogram, one workgroup");
static_assert(CH_LBINS >= 3 && CH_LBINS <= 2048, "the packed counters flush into bins 1 and 2; the bypass is testable at N <= 2049");
static_assert(CHS_WAVE * CHS_CH_WORD < (1 << 16), "the short chords of a wavefront's words fit a 16-bit counter");
static_assert(CHS_CH_WORDS == 6 * 4, "six words per (phase, direction)");

typedef long long ch_i64;
typedef unsigned long long ch_u64;
static_assert(sizeof(ch_i64) == sizeof(int64_t), "the result words are int64");

// ---- phase 1 ---------------------------------------------------------------------------------------------------------
// grid (column strips, bands).  Thread tid owns column blockIdx.x CH_THREADS + tid and the band's 64 rows of it; its
// wavefront owns the 64 columns of word j / 64 of the rows.
template <typename T, bool NT>
__global__ __launch_bounds__(CH_THREADS) void k_ch_mask(const void* Uv, int N, int nb, double t, ch_u64* __restrict__ cols,
                                                        ch_u64* __restrict__ rows) {
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int j = blockIdx.x * CH_THREADS + threadIdx.x, i0 = blockIdx.y * CHS_CH_WORD;
  const int lane = threadIdx.x % CHS_WAVE, w = j / CHS_CH_WORD;   // (w is the same for the whole wavefront)
  const bool inside = j < N;
  const T CHS_GLOBAL* col = U + (inside ? j : N - 1);
  ch_u64 cw = 0, rw = 0;
#pragma unroll 8
  for (int r = 0; r < CHS_CH_WORD; ++r) {
    const int i = i0 + r;
    const T CHS_GLOBAL* src = col + (size_t)(i < N ? i : N - 1) * N;
    const T x = NT ? __builtin_nontemporal_load(src) : *src;
    const bool p0 = inside && i < N && chs_cc::fg_of((double)x, t, 0);
    cw |= (ch_u64)(p0 ? 1 : 0) << r;
    const ch_u64 b = __ballot(p0);   // (every lane of the wavefront is here: nothing above branches)
    rw = lane == r ? b : rw;
  }
  if (inside) cols[(size_t)blockIdx.y * N + j] = cw;
  if (w < nb && i0 + lane < N) rows[(size_t)w * N + i0 + lane] = rw;
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------
// grid (line groups, 2, nb): blockIdx.y is the direction, blockIdx.z the word k, thread tid owns word k of line
// blockIdx.x CH_GROUP + tid.  hist is [phase][dir][cls][nbins]; the workgroup's LDS histogram [phase][cls][CH_LBINS].
__device__ __forceinline__ void ch_emit(int phase, int len, int cls, int dir, int nbins, ch_u64& packed, int* lh,
                                        ch_u64* __restrict__ hist) {
  if (cls == CHS_CH_INNER && len <= 2) packed += (ch_u64)1 << (16 * ((len - 1) * 2 + phase));
  else if (len < CH_LBINS) atomicAdd(&lh[(phase * 2 + cls) * CH_LBINS + len], 1);
  else if (len < nbins) atomicAdd(&hist[(size_t)((phase * 2 + dir) * 2 + cls) * nbins + len], (ch_u64)1);
}

__global__ __launch_bounds__(CH_GROUP) void k_ch_walk(const ch_u64* __restrict__ planes, int N, int nb, int nbins,
                                                      ch_u64* __restrict__ hist, int* __restrict__ words) {
  __shared__ int lh[4 * CH_LBINS];
  for (int i = threadIdx.x; i < 4 * CH_LBINS; i += CH_GROUP) lh[i] = 0;
  __syncthreads();
  const int dir = blockIdx.y, k = blockIdx.z, line = blockIdx.x * CH_GROUP + threadIdx.x;
  ch_u64 packed = 0;   // four 16-bit counters: the inner chords of length 1 and 2 of either phase (64 chords a word at most)
  if (line < N) {
    const ch_u64* __restrict__ plane = planes + (size_t)dir * nb * N + line;
    const bool last = k == nb - 1;
    // the word, the one behind it and the first CH_BACK before it: loaded whatever the word says, clamped to the line
    const ch_u64 x = plane[(size_t)k * N], nx = plane[(size_t)(last ? k : k + 1) * N];
    ch_u64 m[CH_BACK];
#pragma unroll
    for (int j = 0; j < CH_BACK; ++j) m[j] = plane[(size_t)(k - 1 - j > 0 ? k - 1 - j : 0) * N];
    const int left = N - k * CHS_CH_WORD, nbits = left < CHS_CH_WORD ? left : CHS_CH_WORD;   // (>= 1)
    int q = (int)(x & 1), err = 0;   // q: the bit of the current run (1 is phase 0)
    ch_u64 z = q ? ~x : x;           // the run goes on while the bits are 0
    int n0 = z ? __ffsll((ch_i64)z) - 1 : CHS_CH_WORD;
    n0 = n0 < nbits ? n0 : nbits;
    const bool goes_on = !last && (int)(nx & 1) == q;   // (of a run that reaches the word's end)
    if (n0 < nbits || !goes_on) {
      // The chord of the word's first pixel ends in this word: how far back does it begin?  A word of the run's phase
      // alone is 64 pixels more; the first other word ends the search with its leading pixels.  k words at the most.
      int len0 = 0, top = k - 1;
      bool open = true;
#pragma unroll 1
      for (int pass = 0; pass < nb / CH_BACK + 2; ++pass) {   // top falls by CH_BACK a pass from k - 1 < nb: the cap is never used up
        if (top < 0 || !open) break;
        if (pass > 0) {
#pragma unroll
          for (int j = 0; j < CH_BACK; ++j) m[j] = plane[(size_t)(top - j > 0 ? top - j : 0) * N];
        }
#pragma unroll
        for (int j = 0; j < CH_BACK; ++j) {
          if (open && top - j >= 0) {
            const ch_u64 zz = q ? ~m[j] : m[j];
            if (zz) { len0 += __clzll((ch_i64)zz); open = false; }
            else len0 += CHS_CH_WORD;
          }
        }
        top -= CH_BACK;
      }
      if (open && top >= 0) err |= CH_ERR_WALK;
      // (open: no change back to the line's start: the chord begins at the wall)
      ch_emit(q ^ 1, len0 + n0, (open || (n0 == nbits && last)) ? CHS_CH_CUT : CHS_CH_INNER, dir, nbins, packed, lh, hist);
    }
    if (n0 < nbits) {
      int pos = n0;
      bool done = false;
      q ^= 1; z = ~z;
#pragma unroll 1
      // Every pass moves pos on by one at least (the bit at pos of the flipped word is 0) and ends the loop once pos
      // reaches nbits <= 64: 64 passes at the most, the cap is never used up.
      for (int it = 0; it < CHS_CH_WORD + 2; ++it) {
        const ch_u64 y = z >> pos;   // (pos < nbits <= 64)
        int n = y ? __ffsll((ch_i64)y) - 1 : CHS_CH_WORD;
        n = n < nbits - pos ? n : nbits - pos;
        pos += n;
        if (pos >= nbits) {   // the run reaches the word's end: it is this word's if it ends here
          if (last) ch_emit(q ^ 1, n, CHS_CH_CUT, dir, nbins, packed, lh, hist);
          else if ((int)(nx & 1) != q) ch_emit(q ^ 1, n, CHS_CH_INNER, dir, nbins, packed, lh, hist);
          done = true;
          break;
        }
        ch_emit(q ^ 1, n, CHS_CH_INNER, dir, nbins, packed, lh, hist);
        q ^= 1; z = ~z;
      }
      if (!done) err |= CH_ERR_WALK;
    }
    if (err) atomicOr(&words[CH_W_ERR], err);
  }
  // the short chords of a wavefront in one add per counter (64 lanes x 64 chords stay below 2^16)
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) packed += __shfl_xor(packed, off);
  if (threadIdx.x % CHS_WAVE == 0) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {   // c4 = (len - 1) 2 + phase
      const int c = (int)((packed >> (16 * c4)) & 0xffff);
      if (c) atomicAdd(&lh[((c4 & 1) * 2 + CHS_CH_INNER) * CH_LBINS + (c4 >> 1) + 1], c);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * CH_LBINS; i += CH_GROUP) {
    const int c = lh[i];
    const int pc = i / CH_LBINS, len = i % CH_LBINS;   // pc = phase 2 + cls
    if (c && len < nbins) atomicAdd(&hist[(size_t)(((pc >> 1) * 2 + dir) * 2 + (pc & 1)) * nbins + len], (ch_u64)c);
  }
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------
// One workgroup; CH_FIN_THREADS / 8 threads per histogram (two wavefronts), a shuffle tree inside the wavefront, thread
// 0 joins the sixteen partials in a fixed order and checks the look.
struct ChSum {
  ch_i64 n, s, s2, mx;
};

__global__ __launch_bounds__(CH_FIN_THREADS) void k_ch_fin(const ch_u64* __restrict__ hist, int N, int nbins, ch_i64* __restrict__ out,
                                                           int* __restrict__ words) {
  constexpr int PER = CH_FIN_THREADS / CH_HISTS;
  __shared__ ChSum red[CH_FIN_THREADS / CHS_WAVE];
  const int h = threadIdx.x / PER;   // h = (phase 2 + dir) 2 + cls
  ChSum s{0, 0, 0, 0};
  for (int c = threadIdx.x % PER; c < nbins; c += PER) {
    const ch_i64 n = (ch_i64)hist[(size_t)h * nbins + c];
    s.n += n; s.s += n * c; s.s2 += n * c * (ch_i64)c;
    if (n > 0 && c > s.mx) s.mx = c;
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) {
    s.n += __shfl_down(s.n, off); s.s += __shfl_down(s.s, off); s.s2 += __shfl_down(s.s2, off);
    const ch_i64 o = __shfl_down(s.mx, off);
    s.mx = o > s.mx ? o : s.mx;
  }
  if (threadIdx.x % CHS_WAVE == 0) red[threadIdx.x / CHS_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    ch_i64 pixels[2] = {0, 0}, cut[2] = {0, 0};
    for (int g = 0; g < CH_HISTS; ++g) {
      ChSum t{0, 0, 0, 0};
      for (int v = g * (PER / CHS_WAVE); v < (g + 1) * (PER / CHS_WAVE); ++v) {
        t.n += red[v].n; t.s += red[v].s; t.s2 += red[v].s2; t.mx = red[v].mx > t.mx ? red[v].mx : t.mx;
      }
      const int dir = (g >> 1) & 1;
      ch_i64* o = out + 6 * (g >> 1);
      if ((g & 1) == CHS_CH_INNER) { o[CHS_CH_N_INNER] = t.n; o[CHS_CH_SUM_INNER] = t.s; o[CHS_CH_SUM2_INNER] = t.s2; o[CHS_CH_MAX_INNER] = t.mx; }
      else { o[CHS_CH_N_CUT] = t.n; o[CHS_CH_SUM_CUT] = t.s; cut[dir] += t.n; }
      pixels[dir] += t.s;
    }
    int err = 0;
    for (int dir = 0; dir < 2; ++dir) {
      if (pixels[dir] != (ch_i64)N * N) err |= CH_ERR_SUM;
      if (cut[dir] < N || cut[dir] > 2 * (ch_i64)N) err |= CH_ERR_CUT;
    }
    if (err) atomicOr(&words[CH_W_ERR], err);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct ChResult {   // pinned
  int words[CH_NW];
  ch_i64 out[CHS_CH_WORDS];
};

struct ChBuf : LookBase {   // have: hist is the look's snapshot
  int nb = 0, nbins = 0;
  ch_u64* planes = nullptr;     // [2][nb][N]: the column plane (the words of the columns), then the row plane
  ch_u64* hist = nullptr;       // [2][2][2][nbins]
  ch_i64* out = nullptr;        // [CHS_CH_WORDS]
  int* words = nullptr;         // [CH_NW]
  ChResult* hRes = nullptr;
};

void ch_release(ChBuf* s) {
  if (!s) return;
  hipFree(s->planes); hipFree(s->hist); hipFree(s->out); hipFree(s->words);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int ch_alloc(ChBuf* s) {
  const int N = s->N;
  s->nb = (N + CHS_CH_WORD - 1) / CHS_CH_WORD;
  s->nbins = chs_chords_bins(N);
  CHS_HIP(hipMalloc(&s->planes, sizeof(ch_u64) * 2 * (size_t)s->nb * N));
  CHS_HIP(hipMalloc(&s->hist, sizeof(ch_u64) * CH_HISTS * (size_t)s->nbins));
  CHS_HIP(hipMalloc(&s->out, sizeof(ch_i64) * CHS_CH_WORDS));
  CHS_HIP(hipMalloc(&s->words, sizeof(int) * CH_NW));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(ChResult), hipHostMallocDefault));
  return CHS_OK;
}

template <typename T>
int launch_mask(const ChBuf* s, const void* U, double t, hipStream_t st) {
  const int N = s->N;
  ch_u64* cols = s->planes + (size_t)CHS_CH_COLS * s->nb * N;
  ch_u64* rows = s->planes + (size_t)CHS_CH_ROWS * s->nb * N;
  const dim3 grid((N + CH_THREADS - 1) / CH_THREADS, s->nb);
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  if (chs_grid_exceeds_cache((size_t)N, sizeof(T))) k_ch_mask<T, true><<<grid, CH_THREADS, 0, st>>>(U, N, s->nb, t, cols, rows);
  else k_ch_mask<T, false><<<grid, CH_THREADS, 0, st>>>(U, N, s->nb, t, cols, rows);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

int ch_run(ChBuf* s, Engine* E, hipStream_t st, double t, const std::string& who) {
  const int N = s->N;
  look_forget(s);
  CHS_HIP(hipMemsetAsync(s->words, 0, sizeof(int) * CH_NW, st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(ch_u64) * CH_HISTS * (size_t)s->nbins, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  const int rc = E->dtype == CHS_F64 ? launch_mask<double>(s, E->dU, t, st) : launch_mask<float>(s, E->dU, t, st);
  if (rc) return rc;
  k_ch_walk<<<dim3((N + CH_GROUP - 1) / CH_GROUP, 2, s->nb), CH_GROUP, 0, st>>>(s->planes, N, s->nb, s->nbins, s->hist, s->words);
  CHS_HIP(hipGetLastError());
  k_ch_fin<<<1, CH_FIN_THREADS, 0, st>>>(s->hist, N, s->nbins, s->out, s->words);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * CH_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(s->hRes->out, s->out, sizeof(ch_i64) * CHS_CH_WORDS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const int err = s->hRes->words[CH_W_ERR];
  if (err) {
    std::string m;
    if (err & CH_ERR_WALK) m += " a loop of k_ch_walk (the runs of a word, the search backwards) reached its cap;";
    if (err & CH_ERR_SUM) m += " the chords of a direction do not add up to N^2 pixels;";
    if (err & CH_ERR_CUT) m += " the cut chords of a direction are not N to 2 N;";
    chs_set_error(who + ": self-check failed:" + m);
    return CHS_ECHECK;
  }
  return look_end(s);
}
}  // namespace

void chs_ch_free(void** buf) {
  if (!buf) return;
  ch_release((ChBuf*)*buf);
  *buf = nullptr;
}

void chs_ch_forget(void* buf) {
  if (buf) look_forget((ChBuf*)buf);
}

int chs_ch_look(Engine* E, hipStream_t st, void** buf, double threshold, int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if ((rc = look_check_field(E, CH_MAX_N, who))) return rc;
  if ((rc = look_buffers<ChBuf>(buf, E->N, ch_alloc, ch_release))) return rc;
  ChBuf* s = (ChBuf*)*buf;
  if ((rc = ch_run(s, E, st, threshold, who))) return rc;
  memcpy(out, s->hRes->out, sizeof(int64_t) * CHS_CH_WORDS);
  return CHS_OK;
}

int chs_ch_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const ChBuf* s = (const ChBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * CH_HISTS * (size_t)nbins);
}

extern "C" int32_t chs_chords_bins(int32_t N) { return N < 1 ? 0 : N + 1; }

extern "C" int chs_chords(chs_handle h, double threshold, int64_t out[CHS_CH_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_chords: null handle"); return CHS_EINVAL; }
  return chs_ch_look(E, E->stream, &E->ch, threshold, out, "chs_chords");
}

extern "C" int chs_chords_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_chords_hist: null handle"); return CHS_EINVAL; }
  return chs_ch_hist(E->ch, E->hc.device, E->stream, nbins, out, "chs_chords_hist");
}

extern "C" int chs_chords_last_ms(chs_handle h, double* ms) {
  return look_last_ms(h, h ? (const ChBuf*)((Engine*)h)->ch : nullptr, ms, "chs_chords");
}

extern "C" int chs_chords_tile(int32_t* word_bits, int32_t* lines_per_group, int32_t* local_bins) {
  if (!word_bits || !lines_per_group || !local_bins) { chs_set_error("chs_chords_tile: null argument"); return CHS_EINVAL; }
  *word_bits = CHS_CH_WORD;
  *lines_per_group = CH_GROUP;
  *local_bins = CH_LBINS;
  return CHS_OK;
}
