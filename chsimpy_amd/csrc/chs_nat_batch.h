// chs_nat_batch.h -- the member record of a batch of natural-order engines (chs_batch.hip: a batch of chirp members).
//
// The natural step (chs_api.hip: one_step) is thirteen unfused launches -- k_mu, k_pre, dct2d (two line kernels, two
// transposes), k_spectral, dct2d again, k_diag, k_fin -- each of which returns at once on st->halt and none of which is
// fused with its neighbours: the member becomes the slowest grid dimension.  The batched instantiations of those kernels
// (chs_pointwise.hip, chs_chirp_batch.hip) are the single handle's kernels with one argument more, a NatSel, as the
// batched kernels of the fast engine are (chs_fast_kernels.h: an empty pack is the single handle's kernel, the same
// code as before; `if constexpr` adds the batch part): a workgroup reads its member's record (uniform, through the
// constant address space: scalar loads), takes the member's arrays, state and constants in place of the arguments and
// runs the one body.  Block shapes, grid.x, band sizes and reduction trees are the single handle's, so a member's
// partial sums, and with them its record, are the single handle's bit for bit.
#pragma once
#include "chs_common.h"

// the member's five N x N arrays, as NatSel::src / dst select them
enum { NAT_U = 0, NAT_MU = 1, NAT_T1 = 2, NAT_T2 = 3, NAT_HAT = 4, NAT_ARRAYS = 5 };

struct NatMember {
  DevConsts dc;
  DevState* st;
  long long nsteps;        // iterations of the running call: the member's step of a launch is st->rows_written
  void* arr[NAT_ARRAYS];   // U, MU, T1, T2, hat (NAT_*)
  double* partMu;          // [nBands] k_mu -> k_pre
  double* partDiag;        // [nDiagBlocks][4] k_diag -> k_fin
  double* rows;            // the member's ring of timedata rows
  long long rowsCap;
};
static_assert(sizeof(NatMember) % 8 == 0, "records are read in 8-byte words");

// what a batched launch passes behind the single kernel's arguments
struct NatSel {
  const NatMember* mem;    // device array of the records, indexed by the grid's slowest dimension
  int src, dst;            // the arrays a transform kernel reads and writes (NAT_*)
};

typedef const __attribute__((address_space(4))) NatMember ConstNatMember;
__device__ __forceinline__ ConstNatMember& nat_member(const NatSel& s, unsigned member) {
  return ((ConstNatMember*)s.mem)[member];
}
// Participation: a workgroup leaves at once when its member has halted or has no step left in this call.  Only k_fin
// advances rows_written, so all thirteen kernels of a step agree; a member with nsteps = 0 sits the call out.
__device__ __forceinline__ bool nat_sits_out(ConstNatMember& m) {
  const DevState* st = m.st;
  return st->halt != 0 || st->rows_written >= m.nsteps;
}

// ---- batched launchers: every one a single launch over all B records ------------------------------------------------
// (chs_pointwise.hip; E0 = member 0: all members share N, the element type, the band counts and the eigenvalue table)
int chs_nat_batch_mu(Engine* E0, hipStream_t s, const NatMember* mem, int B);        // grid (nBands, B)
int chs_nat_batch_pre(Engine* E0, hipStream_t s, const NatMember* mem, int B);       // grid B
int chs_nat_batch_spectral(Engine* E0, hipStream_t s, const NatMember* mem, int B);  // grid (blocks, B): hat, T2
int chs_nat_batch_diag(Engine* E0, hipStream_t s, const NatMember* mem, int B);      // grid (x, y, B)
int chs_nat_batch_fin(Engine* E0, hipStream_t s, const NatMember* mem, int B);       // grid B
// (chs_chirp_batch.hip) arr[dst] = dctn / idctn(arr[src]) of every member, arr[tmp] the scratch: four launches with
// member 0's tables; chs_chirp_batch_init raises the batched line kernels' dynamic-LDS limit, once per batch
int chs_chirp_batch_init(Engine* E0);
int chs_chirp_batch_dct2d(Engine* E0, hipStream_t s, const NatMember* mem, int B, int src, int dst, int tmp, bool inverse);
