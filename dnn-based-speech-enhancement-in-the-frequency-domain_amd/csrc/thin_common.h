// What the frame-staged kernels (thin_mask.hip, thin_stage.hip, thin_wgrad.hip) share: two device helpers and the opening checks of their form
// predicates.  The kernels' frame rings, LDS-DMA set-up and epilogues stay with each kernel.
#pragma once
#include "dev_common.h"

namespace sefd {

// every accumulator through ONE statement behind 16 wait states before the epilogue packs it in inline assembly, which the compiler's MFMA hazard padding does not see
__device__ __forceinline__ void settle(f32x4& a, f32x4& b) { asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void settle(f32x4& a, f32x4& b, f32x4& c, f32x4& e) { asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a), "+v"(b), "+v"(c), "+v"(e)); }

// x moved between lanes by the DPP control CTRL (row shifts, quad permutes); a lane without a source reads 0
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}

// The output rows start, and step by frame, position and batch item, at multiples of 8 elements: 16-byte stores (RUNGEMM) or 16-byte LDS-DMA chunks (WGRAD)
inline bool y_strides_aligned(const RunGemm& d) { return d.y_fstride % 8 == 0 && d.y_off % 8 == 0 && d.y_tstride % 8 == 0 && d.y_bstride % 8 == 0; }

// What every RUNGEMM form starts from: bf16 in and out, 16-byte aligned runs and output rows, a plain epilogue
inline bool thin_plain_bf16(const RunGemm& d) {
  if (d.xdt != DT_BF16 || d.ydt != DT_BF16 || !(d.flags & kRunAligned) || !(d.flags & kRunYAligned)) return false;
  if (d.flags & (kRunAccum | kRunRelu | kRunBnBwd | kRunWTile32 | kRunEnc0 | kRunDyFromBn | kRunRank)) return false;
  return y_strides_aligned(d) && d.ldw % 8 == 0;
}

}  // namespace sefd
