// The LDS-DMA tile ring of maxsim.hip's ring kernels and dsh_scores_kernel (dense_small_hi.hip), device only: the casts and
// the issue of an LDS-DMA, the s_waitcnt immediates, the waits.  (Its addresses: tile_swizzle.hpp.  dense_panel.hip, a
// double buffer with its own publish step, takes the casts only.)  Where a wave's MFMAs of a tile take less than one trip
// to L2, the tiles go through a RING of NBUF LDS stages filled by LDS-DMA (global_load_lds_dwordx4: no staging registers,
// no ds_write), NBUF - 1 tiles ahead of the one being multiplied:
//   step s:  s_waitcnt lgkmcnt(0) vmcnt(PIECES x tiles in flight behind tile s)   this wave's pieces of tile s have landed
//            s_barrier                                                       ... everybody's; tile s - 1 has been read
//            DMA of tile s + NBUF - 1 into the stage of tile s - 1
//            ds_reads of tile s; the MFMAs
// One raw barrier per tile and no vmcnt(0) in the loop (a __syncthreads() would drain the DMAs in flight); the waits
// are the s_waitcnt BUILTIN, not inline asm: hipcc's own wait-count pass must see them, or it re-waits in front of
// the MFMAs.  A DMA lands lane-linear (stage base + lane * 16): the XOR swizzle that makes the ds_read_b128 fragment
// reads conflict-free is applied to the per-lane SOURCE address (piece_offs; dense_panel.hip does the same).
#pragma once
#include "tile_swizzle.hpp"

namespace amdr {

#define AMDR_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define AMDR_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

// this wave's pieces of the tile at `src` (wave-uniform; poff: piece_offs) into `dst` = the stage + its first piece's KiB
template <int PIECES>
__device__ __forceinline__ void ring_issue_tile(const unsigned char* src, const long (&poff)[PIECES], unsigned char* dst) {
#pragma unroll
  for (int u = 0; u < PIECES; ++u)
    __builtin_amdgcn_global_load_lds(AMDR_GPTR(src + poff[u]), AMDR_LPTR(dst + u * 1024), 16, 0, 0);
}

// The waits.  simm16 on gfx9: vmcnt [3:0] (+ [15:14]), expcnt [6:4] (7 = none), lgkmcnt [11:8] (15 = none).
constexpr int waitcnt_imm(int vm, int exp, int lgkm) { return (vm & 15) | ((vm >> 4) << 14) | (exp << 4) | (lgkm << 8); }
constexpr int vmcnt_imm(int n) { return waitcnt_imm(n, 7, 15); }  // vmcnt(n) alone
constexpr int kLgkm0 = waitcnt_imm(63, 7, 0);                     // lgkmcnt(0) alone
static_assert(vmcnt_imm(0) == 0x0F70 && vmcnt_imm(2) == 0x0F72 && vmcnt_imm(4) == 0x0F74 && vmcnt_imm(6) == 0x0F76 &&
              vmcnt_imm(16) == 0x4F70 && kLgkm0 == 0xC07F, "the immediates the kernels once carried by hand");
__device__ __forceinline__ void wait_vm0() { __builtin_amdgcn_s_waitcnt(vmcnt_imm(0)); }  // every load and DMA of this wave
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(kLgkm0); }      // its LDS reads: a stage may be refilled
// This wave's pieces of a tile have landed once at most PIECES x (tiles issued behind it) requests are outstanding:
// vmcnt(PIECES x min(behind, CAP)) (fewer than the truth only makes the wait stricter; so do other loads issued meanwhile).
template <int PIECES, int CAP, int B = CAP>
__device__ __forceinline__ void wait_vm(int behind) {
  static_assert(PIECES * CAP < 64, "vmcnt has 6 bits");
  if constexpr (B == 0) {
    wait_vm0();
  } else {
    if (B == CAP ? behind >= B : behind == B)
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(PIECES * B));
    else
      wait_vm<PIECES, CAP, B - 1>(behind);
  }
}
// lgkmcnt(0) as ONE unconditional instruction: inside the branches the wait-count pass still re-waited before the MFMAs
template <int PIECES, int CAP>
__device__ __forceinline__ void wait_tile(int behind) {
  wait_lgkm0();
  wait_vm<PIECES, CAP>(behind);
}

}  // namespace amdr
