// Device primitives shared by the gfx950 kernels: the inline-asm wrappers and the few builtin forms that go with them.
// Every asm wrapper encodes a hardware rule -- a register class, a load the compiler must not count and the wait that answers it,
// a wait state inside the string.  The rule stands in the comment above the wrapper, once, and the kernels call the wrapper.
#pragma once
#include "common.h"

namespace cyk {

typedef int i32x4 __attribute__((ext_vector_type(4)));     // a buffer descriptor (4 SGPRs)

// ---- matrix cores, fp32
// More accumulator tiles than the AGPR file holds (18 x 16 or 36 x 2 x 4 = 288 registers against 256): left to itself the
// compiler shuttles accumulators between the two files in every chunk (288 v_accvgpr_write per chunk measured).  The MFMAs are
// therefore written with an explicit register class: _a accumulates in place in AGPRs, _v in arch VGPRs.
// hipcc does not look inside an asm statement and gfx950 does not interlock an MFMA with the first access of its destination:
// the software wait states behind these are the caller's (tools/check_mfma_hazards.py counts them in the emitted code).
__device__ __forceinline__ void mfma16_a(f32x4& c, float a, float b) {
  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_v(f32x4& c, float a, float b) {
  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma32_a(f32x16& c, float a, float b) {
  asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma32_v(f32x16& c, float a, float b) {
  asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// the tracked form: the compiler allocates the accumulator and pads the hazards itself
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// an accumulator tile zeroed by the matrix pipe (C = the inline constant 0), born in AGPRs: no 16 v_accvgpr_write
__device__ __forceinline__ f32x16 mfma32_zero() {
  f32x16 c;
  asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %1, 0" : "=a"(c) : "v"(0.f));
  return c;
}
// One accumulator element, read where the statement stands.  Plain `acc[xi][r]` lets the compiler copy ALL 16
// accumulator vectors AGPR -> VGPR in front of the output transform (256 VGPRs: everything else is spilled).
__device__ __forceinline__ float acc_elem(float a_elem) {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x) : "a"(a_elem));
  return x;
}

// ---- packed fp32 arithmetic
// as plain vector expressions: hipcc selects v_pk_fma_f32 / v_pk_add_f32 for them on gfx950 (with inline
// constants and neg modifiers), and -- unlike inline-asm statements -- needs no s_nop pad between two dependent ones
__device__ __forceinline__ f32x2 pkfma(f32x2 x, f32x2 y, f32x2 z) { return __builtin_elementwise_fma(x, y, z); }    // x * y + z
__device__ __forceinline__ f32x2 pkfnma(f32x2 x, f32x2 y, f32x2 z) { return __builtin_elementwise_fma(-x, y, z); }  // z - x * y
__device__ __forceinline__ f32x2 pkadd(f32x2 x, f32x2 y) { return x + y; }
__device__ __forceinline__ f32x2 pksub(f32x2 x, f32x2 y) { return x - y; }
// forced: two fp32 operations in one VALU instruction (the compiler splits most float2 adds into two v_add_f32)
__device__ __forceinline__ f32x2 asm_pk_add(f32x2 x, f32x2 y) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ f32x2 asm_pk_sub(f32x2 x, f32x2 y) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ f32x2 asm_pk_fma(f32x2 x, f32x2 y, f32x2 z) {
  f32x2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}

// ---- vector memory the compiler does not count (V: any 16-byte vector type)
// A load tracked by hipcc and pending at a loop header draws vmcnt(0) there (the join of the loop's back edge with its entry),
// i.e. a wait for the loads issued in the loop's last slots.  These loads are therefore invisible to the compiler and waited
// for by hand: vmwait<N> in front of the first use, N = the EXACT number of vector-memory operations the schedule issues
// between the load and that use (the counter retires in order: a flat, larger count makes an old load wait for younger ones,
// i.e. for HBM latency; tools/check_vmcnt.py replays the emitted stream against the counts).  The wait is tied to the register
// it answers ("+v"), so neither the compiler nor the scheduler moves the first use in front of it.
template <int OFF, typename V> __device__ __forceinline__ void gload(V& dst, const char* base, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(OFF));
}
// ... through a buffer descriptor: an item outside the image gets an offset beyond num_records and the hardware's range check
// returns zeros -- no select, no zero page, no masks; a uniform offset travels as the instruction's scalar offset (no vector add).
template <typename V> __device__ __forceinline__ void bufload(V& dst, i32x4 desc, unsigned voff, unsigned soff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(desc), "s"(soff));
}
// (the s_nop: a vector-memory store of more than 64 bits reads its data registers a cycle behind its issue, and a vector instruction
// that overwrites them right away needs a wait state in between -- hipcc pads it for its own stores and cannot for an asm statement:
// without it the first dword of now and then a stored piece was the NEXT item's LDS address, computed into the same register)
template <typename V> __device__ __forceinline__ void bufstore(const V& src, i32x4 desc, unsigned voff, unsigned soff) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" : : "v"(src), "v"(voff), "s"(desc), "s"(soff) : "memory");
}
template <int N, typename V> __device__ __forceinline__ void vmwait(V& x) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(x) : "n"(N)); }
// descriptor of the `bytes` bytes at p: base (48 bits) and stride 0 in words 0 / 1, num_records = bytes, word 3 = DATA_FORMAT 32.
// Raw buffer: the range check compares the byte offset (voff + the instruction's immediate) with num_records.
__device__ __forceinline__ i32x4 bufdesc(const void* p, unsigned bytes) {
  const unsigned long long b = (unsigned long long)(uintptr_t)p;
  return i32x4{(int)(unsigned)b, (int)(unsigned)((b >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

// ---- LDS
// (dword[O0 * 64], dword[O1 * 64]) from LDS byte address `addr` as ONE aligned register pair.  Plain C++ loads
// are paired up by the compiler as it likes (adjacent columns) and then shuffled with v_mov + an immediate wait;
// the weight-gradient transforms need (column c, column c + 2).  The compiler does not count this read: the consumer slot
// waits with an explicit s_waitcnt.
template <int O0, int O1> __device__ __forceinline__ f32x2 lds_pair_st64(unsigned addr) {
  f32x2 r;
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(r) : "v"(addr), "n"(O0), "n"(O1));
  return r;
}

}  // namespace cyk
