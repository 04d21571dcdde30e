// chs_look.h -- what the looks at the field have in common (chs_spectrum, chs_morphology, chs_components, chs_distance,
// chs_chords, chs_composition .hip): how a kernel loads the field, and the host side's bracket
// around a look.
// Only what is textually the same in those files is here; what a look allocates, launches and checks is its own.
#pragma once
#include <cmath>
#include <new>

#include "chs_common.h"

// ---- device side -----------------------------------------------------------------------------------------------------
// The field's address comes out of a record in memory or a void*, where the compiler knows nothing of it and would load
// through flat instructions -- which count as LDS traffic too, so that every wait for LDS or a cross-lane move would wait
// for the field on its way as well.  It is device memory: say so.
#define CHS_GLOBAL __attribute__((address_space(1)))

typedef double chs_d2 __attribute__((ext_vector_type(2)));
typedef float chs_f4 __attribute__((ext_vector_type(4)));

// 16 bytes of T
template <typename T> struct ChsVec;
template <> struct ChsVec<double> { typedef chs_d2 type; static constexpr int V = 2; };
template <> struct ChsVec<float> { typedef chs_f4 type; static constexpr int V = 4; };

// x[0 .. V) <- src[0 .. V): one element, or the 16 bytes of ChsVec<T> in one load (src is then 16-byte aligned).  NT: a
// non-temporal load, for a read-once sweep over a field that exceeds the cache.  (k_dt_mask of chs_distance.hip holds
// this text written out: a change here goes there too.)
template <typename T, int V, bool NT>
__device__ __forceinline__ void chs_load(const T CHS_GLOBAL* src, T (&x)[V]) {
  if constexpr (V == 1) {
    x[0] = NT ? __builtin_nontemporal_load(src) : *src;
  } else {
    static_assert(V == ChsVec<T>::V, "one 16-byte load");
    typedef const typename ChsVec<T>::type CHS_GLOBAL* VP;
    const typename ChsVec<T>::type v = NT ? __builtin_nontemporal_load(reinterpret_cast<VP>(src)) : *reinterpret_cast<VP>(src);
#pragma unroll
    for (int e = 0; e < V; ++e) x[e] = v[e];
  }
}

// The radius bin of the distance look (chs_distance.hip) and of the looks that bin its D2 (chs_skeleton.hip):
// k with k^2 <= v < (k+1)^2 for 0 <= v <= 2^30: the float root is off by one at most, two integer comparisons settle it
__host__ __device__ inline int dt_isqrt(int v) {
  int k = (int)sqrtf((float)v);
  k -= (k * k > v) ? 1 : 0;
  k += ((k + 1) * (k + 1) <= v) ? 1 : 0;
  return k;
}

// ---- host side -------------------------------------------------------------------------------------------------------
// What the buffer set of every look begins with.
struct LookBase {
  int N = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};   // around the kernels of the last look
  double ms = -1.0;                        // their device time; < 0: none to report
  bool have = false;                       // a look has succeeded: the device arrays are its snapshot
};

// The buffer set of a look at grid size N behind *buf: the one that is there, or a new one in its place.  Buf derives from
// LookBase; alloc(s) allocates the look's own arrays and release(s) frees them, the events and s (nullptr: nothing).
template <typename Buf>
int look_buffers(void** buf, int N, int (*alloc)(Buf*), void (*release)(Buf*)) {
  Buf* s = (Buf*)*buf;
  if (s && s->N == N) return CHS_OK;
  release(s);
  *buf = nullptr;
  s = new (std::nothrow) Buf();
  if (!s) { chs_set_error("out of host memory"); return CHS_EINVAL; }
  *buf = s;   // (freed with its owner whatever fails below)
  s->N = N;
  int rc;
  if ((rc = alloc(s))) return rc;
  for (auto& e : s->ev) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

inline void look_release_events(LookBase* s) {
  for (auto e : s->ev) if (e) hipEventDestroy(e);
}

// The argument checks of a thresholded look come in two halves, a look's own (side, connectivity) between them: which
// comes first decides the error of a doubly-wrong call.  Neither touches the last look.
inline int look_check_args(const void* out, double threshold, const std::string& who) {
  if (!out) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!std::isfinite(threshold)) { chs_set_error(who + ": the threshold must be finite"); return CHS_EINVAL; }
  return CHS_OK;
}

inline int look_check_field(const Engine* E, int max_N, const std::string& who) {
  if (E->N > max_N) { chs_set_error(who + ": N above " + std::to_string(max_N)); return CHS_EINVAL; }
  if (!E->have_U) { chs_set_error(who + ": no field (chs_set_U / chs_init_U_pcg64 first)"); return CHS_ESTATE; }
  CHS_HIP(hipSetDevice(E->hc.device));
  return CHS_OK;
}

inline void look_forget(LookBase* s) {
  s->have = false; s->ms = -1.0;
}

// The bracket of a look: look_forget, the look's memsets, ev[0], its kernels, ev[1], the copies of its result words, the
// wait for the stream, its self-check -- and look_end, which takes the time and keeps the look.
inline int look_end(LookBase* s) {
  float ms = 0.f;
  CHS_HIP(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->ms = ms;
  s->have = true;
  return CHS_OK;
}

// A fetch of something the last look left on the device: is there one ...
inline int look_ready(const LookBase* s, const void* out, const std::string& who) {
  if (!out) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!s || !s->have) { chs_set_error(who + ": no look so far"); return CHS_ESTATE; }
  return CHS_OK;
}

// ... and its copy to the host, waited for.
inline int look_fetch(int device, hipStream_t st, void* dst, const void* src, size_t bytes) {
  CHS_HIP(hipSetDevice(device));
  CHS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  return CHS_OK;
}

// chs_X_last_ms of a handle; what = "chs_X"
inline int look_last_ms(const void* h, const LookBase* s, double* ms, const char* what) {
  const std::string who = std::string(what) + "_last_ms";
  if (!h || !ms) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!s || s->ms < 0.0) { chs_set_error(who + ": no " + what + " call so far"); return CHS_ESTATE; }
  *ms = s->ms;
  return CHS_OK;
}
