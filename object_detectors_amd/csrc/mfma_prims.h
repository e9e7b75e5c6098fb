// Primitives every MFMA kernel file shares (gfx950): LDS-DMA through a buffer descriptor, the multiply-shift integer divide, the 16-lane
// row sum, the counted vector-memory wait and the 8-XCD block remap.  One definition each; everything has internal linkage.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// division by a launch-invariant divisor without the ~40-instruction integer divide (n < 2^31; Granlund-Montgomery round-up form).
// A kernel that needs the divisor itself keeps it next to the FastDiv.
struct FastDiv {
  unsigned mul, shift;
};
inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  f.shift = l;
  f.mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv f) { return (__umulhi(f.mul, n) + n) >> f.shift; }

namespace {

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst_uniform) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst_uniform, 16, 0, 0);
}

// LDS-DMA through a buffer descriptor: per-lane 32-bit byte offset + SCALAR offset (the tap / k-step part of the
// address costs no vector instruction); a lane whose voffset is out of range gets zeros written to LDS, which is
// exactly the convolution's zero padding.
// Issued as inline assembly ON PURPOSE: for the builtin the compiler's wait-count pass assumes every later ds_read may alias
// the DMA's LDS destination and puts s_waitcnt vmcnt(0) in front of the next fragment read, which turns every counted wait of
// the ring into a full drain (no load/compute overlap inside a workgroup, whatever the ring depth).  The kernels order DMA and
// reads themselves (counted vmcnt + barrier), so the compiler must not know about the LDS side of these loads.
// Both scalar operands must be wave-uniform AND in scalar registers: a caller whose offset comes out of an integer division (which
// runs on the vector ALU) applies readfirstlane itself.
typedef __attribute__((ext_vector_type(4))) int srd_t;
__device__ __forceinline__ srd_t make_srd(const void* base, unsigned num_records) {
  const unsigned long long a = (unsigned long long)base;
  srd_t r;
  r[0] = (int)(unsigned)a;
  r[1] = (int)((unsigned)(a >> 32) & 0xFFFFu);
  r[2] = (int)num_records;
  r[3] = 0x00020000;
  return r;
}
__device__ __forceinline__ unsigned lds_addr(const void* lds_ptr) {
  return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)lds_ptr;
}
__device__ __forceinline__ void bufld16_at(srd_t rsrc, unsigned lds, int voffset, int soffset) {      // the one statement of the instruction sequence
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory");
}
__device__ __forceinline__ void bufld16(srd_t rsrc, const void* lds_dst_uniform, int voffset, int soffset) {
  bufld16_at(rsrc, lds_addr(lds_dst_uniform), voffset, soffset);
}
#define OOB_VOFF ((int)0x80000000)

// s_waitcnt vmcnt(N): at most N of this wave's vector-memory operations (LDS-DMA pieces, stores) are still in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// sum over the 16 lanes of a DPP row (lanes sharing lane>>4), result in every lane: 4 VALU+DPP ops, no LDS traffic
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
  return v;
}

// XCD-aware block remap: blocks b and b + 8 run on the same XCD, so each of the 8 XCDs gets a contiguous run of tile indices (tiles that
// share an operand tile hit that XCD's L2); bijective for any grid size
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, loc = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

}  // namespace
