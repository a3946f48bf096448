// The exact split-operand arithmetic of the MFMA kernels: the one definition of every primitive the precision contract rests on.
//
// Two arithmetics (template parameter F16 of the kernels that have both):
//   false  three bf16 pieces per fp32 value,  a = a1 + a2 + a3  (a1 = rne(a), a2 = rne(a - a1), a3 = rne(a - a1 - a2): 24 mantissa
//          bits), and a product a*b is the sum of the six partial products of weight >= 2^-16 relative to |a||b|,
//              a3*b1 + a1*b3 + a2*b2 + a2*b1 + a1*b2 + a1*b1        (dropped: a2*b3, a3*b2, a3*b3 <= 3 * 2^-24 |a||b|),
//          each exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16 and added smallest first.  The result carries the rounding
//          of an fp32 convolution (tools/experiments/conv3d_bf16x6.hip measures it against an exact evaluation: max 4.5e-6 / rms
//          4.3e-7 at |y| <= 4.8, a sequential fp32 fma loop 4.7e-6 / 5.1e-7) at 6 / 16 of the bf16 MFMA rate = 2.7 x the fp32 MFMA
//          rate.  Contract: 24 bits for EVERY element, whatever its size next to the rest of its tensor.
//   true   two fp16 pieces (v_cvt_pk_f16_f32, round to nearest even; the remainder a - a1 is exact in fp32), three
//          v_mfma_f32_32x32x16_f16 per product (a1b1, a1b2, a2b1: 2^-22 per product).  fp16's range is narrow: both operands are
//          multiplied by a power of two that brings their tensor's largest magnitude (a device scalar the caller provides:
//          mode_abs_max) to [2^14, 2^15) -- f16_scale_of -- and the accumulators by the inverse, all exact.  Contract: 22 bits down
//          to about 2^-17 of the tensor's maximum; elements further below it lose relative precision.
// Which layers run on which arithmetic is the caller's choice (mode_hip/functional.py: the training step and, by default, inference
// take the fp16 pieces where a layer has them; include/mode_hip.h says how to opt out).
//
// Every split below is EXACT -- its pieces sum to the value in fp32, every remainder is an exact fp32 difference -- so the variants
// compute the same bits.  They differ in the instructions the compiler makes of them and in where its scheduler puts those next to
// the MFMAs, which was measured kernel by kernel: a kernel keeps the form it was tuned with, and moving one to another form is a
// performance change (its device code changes), not a clean-up.  Each variant says why it exists, who uses it, and whether its users
// are compiled with -fno-slp-vectorize (FILE_FLAGS of mode_hip/build.py).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mode {
namespace split {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <bool F16> struct Arith {
  static constexpr int NP = F16 ? 2 : 3;     // pieces per fp32 value
  static constexpr int NTERM = F16 ? 3 : 6;  // MFMAs per product
};

// (a, b) rounded to nearest even into one dword of two bf16 (v_cvt_pk_bf16_f32): a in the low half
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// ---- three bf16 pieces: (a, b) -> the packed pieces of the pair, a == a1 + a2 + a3 and b likewise, exactly

// Both remainders as subtractions, the pair pinned by an empty asm statement.
// (the subtractions of a pair stay scalar: packed into v_pk_add_f32 each costs ~9 cycles of the MATRIX pipe -- packed fp32
// instructions do not overlap with MFMAs on gfx950, plain ones do; tools/experiments/mfma_op_cost.hip)
// Users: conv3d_split, conv2d_split, conv2d_split_wgrad (compiled with -fno-slp-vectorize) and conv3d_split_s2, conv3d_split_deconv,
// conv3d_split_wgrad_s2, sphere_win_* (no per-file flag: there the asm statement alone keeps the pair apart).
// One step of it: returns the pair's next piece and leaves the pair's exact remainders in (a, b).  The spherical kernels call the steps
// one by one, spread over the MFMAs of a tap (their split_a / split_b / split_c).
__device__ __forceinline__ uint32_t split_step_bf16_pinned(float& a, float& b) {
  const uint32_t p = pack2(a, b);
  a = a - __builtin_bit_cast(float, p << 16);
  b = b - __builtin_bit_cast(float, p & 0xffff0000u);
  asm("" : "+v"(a), "+v"(b));
  return p;
}
__device__ __forceinline__ void split3_bf16_pinned(float a, float b, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  p1 = split_step_bf16_pinned(a, b);
  p2 = split_step_bf16_pinned(a, b);
  p3 = pack2(a, b);
}

// One of the pair as a subtraction, the other as fma(-1, piece, value) (the same exact difference): two different operations are not
// packed, and no empty asm statement is needed to keep them apart -- the scheduler's group pattern places plain VALU instructions
// under the MFMAs, an inline-asm node in a chain it left (with everything behind it) for the end of the K-step.
// User: conv3d_split_wgrad (compiled with -fno-slp-vectorize).
__device__ __forceinline__ void split3_bf16_subfma(float a, float b, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  p1 = pack2(a, b);
  const float ra = a - __builtin_bit_cast(float, p1 << 16), rb = __builtin_fmaf(-1.f, __builtin_bit_cast(float, p1 & 0xffff0000u), b);
  p2 = pack2(ra, rb);
  const float sa = ra - __builtin_bit_cast(float, p2 << 16), sb = __builtin_fmaf(-1.f, __builtin_bit_cast(float, p2 & 0xffff0000u), rb);
  p3 = pack2(sa, sb);
}

// ---- two fp16 pieces: (a, b) -> the packed pieces of the pair, a1 = rne(a) and a2 = rne(a - a1) with a - a1 exact in fp32 (a1 + a2 are
// the leading 22 bits of a) and b likewise.  The operands arrive scaled (f16_scale_of).

// The remainders as `a - (float)h` and fma(-1, h, b), no asm statement: the compiler makes v_fma_mix_f32 of them, which reads the fp16
// half in place, as long as the pair is not vectorised -- as <2 x float> the remainders lose v_fma_mix_f32 (two v_cvt_f32_f16 more per
// pair) and become packed fp32 instructions, which do not overlap with MFMAs.  So the users NEED -fno-slp-vectorize.
// Users: conv3d_split, conv3d_split_wgrad.
__device__ __forceinline__ void split2_f16_subfma(float a, float b, uint32_t& p1, uint32_t& p2) {
  const f32x2 v = {a, b};
  const f16x2 h1 = __builtin_convertvector(v, f16x2);
  p1 = __builtin_bit_cast(uint32_t, h1);
  const f32x2 r = {a - (float)h1[0], __builtin_fmaf(-1.f, (float)h1[1], b)};
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}

// Two subtractions, the pair pinned by the empty asm statement of split3_bf16_pinned (same reason).
// Users: conv2d_split, conv2d_split_wgrad (compiled with -fno-slp-vectorize).
__device__ __forceinline__ void split2_f16_pinned(float a, float b, uint32_t& p1, uint32_t& p2) {
  const f32x2 v = {a, b};
  const f16x2 h1 = __builtin_convertvector(v, f16x2);
  p1 = __builtin_bit_cast(uint32_t, h1);
  float ra = a - (float)h1[0], rb = b - (float)h1[1];
  asm("" : "+v"(ra), "+v"(rb));
  const f32x2 r = {ra, rb};
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}

// (round 6) the remainders a - (float)h as ONE instruction each: v_fma_mix_f32 reads the fp16 half in place (1.0 * a - h, the same
// exact difference).  Written as `a - (float)h` it is a v_cvt_f32_f16 + a v_sub_f32 per value -- 40 / 72 / 104 of the 445 / 970 / 1 637
// vector instructions of the spherical forward / input-gradient / weight-gradient loops -- and fma(-1, h, a) is folded back to that
// in a file compiled without -fno-slp-vectorize; the asm statement also does what the empty one of split2_f16_pinned does: it keeps
// the pair's two chains scalar.
// User: sphere_win_* (no per-file flag).
__device__ __forceinline__ void split2_f16_mix(float a, float b, uint32_t& p1, uint32_t& p2) {
  const f32x2 v = {a, b};
  const f16x2 h1 = __builtin_convertvector(v, f16x2);
  p1 = __builtin_bit_cast(uint32_t, h1);
  float ra, rb;
  asm("v_fma_mix_f32 %0, 1.0, %3, -%2 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mix_f32 %1, 1.0, %4, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(ra), "=&v"(rb)
      : "v"(p1), "v"(a), "v"(b));
  const f32x2 r = {ra, rb};
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}

// 2^(14 - floor(log2 m)) for the largest magnitude m of a tensor (m * scale in [2^14, 2^15)); 1 for m = 0; magnitudes below 2^-63 are
// treated as 2^-63 (the tensor is zero for every purpose); Inf / NaN maxima give a finite scale and propagate through the products
__device__ __forceinline__ float f16_scale_of(float m) {
  const unsigned e = min(max((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu, 64u), 254u);
  return m == 0.f ? 1.f : __builtin_bit_cast(float, (268u - e) << 23);
}

// ---- D += A * B on 32 x 32 x 16 fragments of packed pieces (8 per lane and operand), fp32 accumulation
__device__ __forceinline__ f32x16 mfma_bf16(uint4 a, uint4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_f16(uint4 a, uint4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma_split(uint4 a, uint4 b, f32x16 c) {
  if constexpr (F16)
    return mfma_f16(a, b, c);
  else
    return mfma_bf16(a, b, c);
}

// Workgroup barrier that orders LDS accesses only: __syncthreads() also drains the vector-memory counter, i.e. waits for the weight
// fragments already requested for the next chunk and for the output stores of a finished tile.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace split
}  // namespace mode
#endif  // __HIPCC__
