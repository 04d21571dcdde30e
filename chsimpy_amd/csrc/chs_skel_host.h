// chs_skel_host.h -- skeleton look: what the kernels of chs_skeleton.hip and the host model
// tests/skel_model.cpp share.  No HIP in here: the per-word functions of the thinning and of the statistics, in plain
// boolean algebra on 64-bit words, 64 pixels at a time.
//
// The plane.  A row of N pixels is W = ceil(N / 64) words; bit j of word w is column 64 w + j; the bits at or beyond N
// are zero and stay zero.  A function below takes the 3 x 3 words about the one it works on -- above, own row, below;
// left, centre, right -- a word outside the plane being 0: everything outside the box is background.
//
// The neighbours of a pixel are x0 .. x7 clockwise from north: N, NE, E, SE, S, SW, W, NW.  North is the row above
// (i - 1), east the next column (j + 1): the east neighbours of a word's pixels are the word shifted DOWN by one bit, the
// bit 0 of the word to the right coming in at the top.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define CHS_SK_HD __attribute__((host)) __attribute__((device)) inline
#else
#define CHS_SK_HD inline
#endif

#define CHS_SK_DIR_N 0
#define CHS_SK_DIR_S 1
#define CHS_SK_DIR_E 2
#define CHS_SK_DIR_W 3

namespace chs_sk {

typedef unsigned long long u64;
static_assert(sizeof(u64) == 8, "a word is 64 pixels");

CHS_SK_HD int words_of(int N) { return (N + 63) / 64; }
// the direction of sub-iteration i = 1, 2, ...: N, S, E, W and again
CHS_SK_HD int dir_of(long long i) { return (int)((i - 1) & 3); }

// the 3 x 3 words about a word: [0] the row above, [1] the word's own, [2] the row below; l, c, r
struct Nine {
  u64 l[3], c[3], r[3];
};

// the eight neighbour planes of the centre word
struct Planes {
  u64 x[8];
};

CHS_SK_HD u64 west_of(u64 l, u64 c) { return (c << 1) | (l >> 63); }   // bit j <- column 64 w + j - 1
CHS_SK_HD u64 east_of(u64 c, u64 r) { return (c >> 1) | (r << 63); }   // bit j <- column 64 w + j + 1

CHS_SK_HD Planes planes_of(const Nine& n) {
  Planes p;
  p.x[0] = n.c[0];
  p.x[1] = east_of(n.c[0], n.r[0]);
  p.x[2] = east_of(n.c[1], n.r[1]);
  p.x[3] = east_of(n.c[2], n.r[2]);
  p.x[4] = n.c[2];
  p.x[5] = west_of(n.l[2], n.c[2]);
  p.x[6] = west_of(n.l[1], n.c[1]);
  p.x[7] = west_of(n.l[0], n.c[0]);
  return p;
}

// the four terms of the Yokoi number: term k / 2 is  not x_k and (x_{k+1} or x_{k+2}),  k = 0, 2, 4, 6
CHS_SK_HD void yokoi_terms(const Planes& p, u64 t[4]) {
  t[0] = ~p.x[0] & (p.x[1] | p.x[2]);
  t[1] = ~p.x[2] & (p.x[3] | p.x[4]);
  t[2] = ~p.x[4] & (p.x[5] | p.x[6]);
  t[3] = ~p.x[6] & (p.x[7] | p.x[0]);
}

// bit j: at least one / at least two of the eight neighbours of pixel j are set
CHS_SK_HD void some_and_two(const Planes& p, u64* some, u64* two) {
  u64 a = 0, b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    b |= a & p.x[k];
    a |= p.x[k];
  }
  *some = a; *two = b;
}

// The pixels of the centre word that sub-iteration direction `dir` deletes: foreground, the neighbour in that direction
// background, Y == 1 (exactly one of the four terms), B >= 2.  A function of the plane before the sub-iteration alone.
CHS_SK_HD u64 deletes(const Nine& n, int dir) {
  const Planes p = planes_of(n);
  u64 t[4];
  yokoi_terms(p, t);
  const u64 two_terms = (t[0] & t[1]) | (t[2] & t[3]) | ((t[0] | t[1]) & (t[2] | t[3]));
  const u64 y1 = (t[0] | t[1] | t[2] | t[3]) & ~two_terms;
  u64 some, two;
  some_and_two(p, &some, &two);
  const u64 toward = p.x[dir == CHS_SK_DIR_N ? 0 : dir == CHS_SK_DIR_S ? 4 : dir == CHS_SK_DIR_E ? 2 : 6];
  return n.c[1] & ~toward & y1 & two;
}

// The pixels of the centre word by what they are in the plane: every mask is a subset of the centre word.
struct Kinds {
  u64 isolated, ends, b2;   // B == 0, B == 1, B >= 2
  u64 y[5];                 // Y == 0 .. 4
  u64 axial_e, axial_s;     // the pixel and its east / south neighbour are both set: every 4-adjacent pair once
  u64 diag_se, diag_sw;     // ... south-east / south-west neighbour: every diagonal pair once
  u64 tri;                  // the 2 x 2 window (pixel, E, S, SE) holds exactly three pixels; bit j stands for the window,
                            // so it is no subset of the centre word
  u64 full;                 // ... all four
};

CHS_SK_HD Kinds kinds_of(const Nine& n) {
  const Planes p = planes_of(n);
  const u64 c = n.c[1];
  Kinds k;
  u64 some, two;
  some_and_two(p, &some, &two);
  k.isolated = c & ~some;
  k.ends = c & some & ~two;
  k.b2 = c & two;
  u64 t[4];
  yokoi_terms(p, t);
  // Y = t0 + t1 + t2 + t3, bit-sliced: two half adders and their sum
  const u64 s01 = t[0] ^ t[1], c01 = t[0] & t[1], s23 = t[2] ^ t[3], c23 = t[2] & t[3];
  const u64 b0 = s01 ^ s23, carry = s01 & s23;
  const u64 b1 = c01 ^ c23 ^ carry, b2 = c01 & c23;   // (c01 and c23: both sums are 0, no carry)
  k.y[0] = c & ~b0 & ~b1 & ~b2;
  k.y[1] = c & b0 & ~b1;
  k.y[2] = c & ~b0 & b1;
  k.y[3] = c & b0 & b1;
  k.y[4] = c & b2;
  k.axial_e = c & p.x[2];
  k.axial_s = c & p.x[4];
  k.diag_se = c & p.x[3];
  k.diag_sw = c & p.x[5];
  const u64 a = c, b = p.x[2], d = p.x[4], e = p.x[3];
  k.full = a & b & d & e;
  k.tri = ((a & b & (d ^ e)) | (d & e & (a ^ b)));
  return k;
}

CHS_SK_HD int popc(u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// The Euler number of a plane at 8-connectivity (8-components minus 4-connected holes of the background) from the sums of
// the word counts: vertices - edges + triangles - tetrahedra of the complex whose simplices are the sets of mutually
// 8-adjacent pixels.  A window of three pixels is one triangle; a full window is four triangles and one tetrahedron.
// It equals (Q1 - Q3 - 2 QD) / 4 of chs_morphology on the same mask.
CHS_SK_HD long long euler8_of(long long pixels, long long axial, long long diagonal, long long tri, long long full) {
  return pixels - axial - diagonal + tri + 3 * full;
}

}  // namespace chs_sk
