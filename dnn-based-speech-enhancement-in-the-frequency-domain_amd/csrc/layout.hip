// Reference layout <-> channels-last at the boundary of a layer that runs on its own (struct NchwCl, sefd_desc.h; planner: plan_layers.cpp).
//
// nchw fp32 [B][C][F][T] has the frames adjacent, cl [B][Tcl][F][Cpad] the channels.  A workgroup owns an LT x LT tile over (channel, frame) of one
// (b, f) and transposes it through a padded [LT][LT + 1] float tile.  LT = 64 (default): a wave moves one whole 256-byte row of frames per instruction on
// the nchw side and rows of 64 channels on the cl side - fp32: 64 lanes x 4 bytes; bf16: 8 lanes x one packed 16-byte chunk of 8 channels, rounded to
// nearest even by v_cvt_pk_bf16_f32.  LT = 32 (knob LAYOUT_TILE=32, read per launch): the [32][33] tile of specconv_kernel (stft_fft.hip), 128-byte rows;
// tools/convlayers_bench.py times both.  ds_write_b32 of row r by lanes tx hits banks ((LT + 1) r + tx) % 32 and the transposed read tile[tx][r] hits
// ((LT + 1) tx + r) % 32 = (tx + r) % 32: conflict-free per 32 lanes.  The chunk accesses (frame r, chunk q) touch banks (r + 8 q + e) % 32.
// nchw -> cl writes the channels C .. Cpad - 1 of every frame it owns as zero (the tile is zero filled where c >= C), so the GEMMs behind it read exact
// zeros against their zero coefficients.  All element offsets are 64-bit.
#include "dev_common.h"
#include "tuning.h"

namespace sefd {
namespace {

template <bool BF, int kLT>                                 // kLT: tile edge, channels and frames
__global__ __launch_bounds__(256) void nchw_cl_kernel(const NchwCl d, const ArenaBases ab) {
  __shared__ float tile[kLT][kLT + 1];
  const int C = d.C, Cp = d.Cpad, F = d.F, T = d.T;
  const int t0 = blockIdx.x * kLT, c0 = blockIdx.y * kLT;
  const int64_t bf = blockIdx.z;
  const int64_t b = bf / F, f = bf - b * F;
  constexpr int kStep = 256 / kLT, kCh = kLT / 8;           // rows per pass of the workgroup; 8-channel chunks per frame
  const int tx = threadIdx.x % kLT, ty = threadIdx.x / kLT;
  float* nchw = reinterpret_cast<float*>(rp(ab, d.nchw));
  char* cl = rp(ab, d.cl);
  const bool to_cl = (d.mode & 1) == 0;
  const int nc = min(kLT, Cp - c0);                          // channels of the tile inside the padded axis (a multiple of 8)
  // element offset of (frame t, channel c) of this (b, f) in cl
  auto cl_at = [&](int t, int c) -> int64_t { return ((b * d.Tcl + t + d.t_off) * F + f) * Cp + c; };
  if (to_cl) {
    for (int r = ty; r < nc; r += kStep) {
      const int c = c0 + r, t = t0 + tx;
      tile[r][tx] = (c < C && t < T) ? nchw[((b * C + c) * F + f) * T + t] : 0.f;
    }
    __syncthreads();
    if constexpr (BF) {
      for (int i = threadIdx.x; i < kLT * kCh; i += 256) {
        const int r = i / kCh, q = i % kCh;                     // frame of the tile, 8-channel chunk
        const int t = t0 + r, c = c0 + 8 * q;
        if (t < T && c < Cp) {                                  // Cpad is a multiple of 8: a chunk is inside or outside as a whole
          uint4 v;
          v.x = pack_bf16x2(tile[8 * q + 0][r], tile[8 * q + 1][r]);
          v.y = pack_bf16x2(tile[8 * q + 2][r], tile[8 * q + 3][r]);
          v.z = pack_bf16x2(tile[8 * q + 4][r], tile[8 * q + 5][r]);
          v.w = pack_bf16x2(tile[8 * q + 6][r], tile[8 * q + 7][r]);
          *reinterpret_cast<uint4*>(cl + cl_at(t, c) * 2) = v;
        }
      }
    } else {
      for (int r = ty; r < kLT; r += kStep) {
        const int t = t0 + r, c = c0 + tx;
        if (t < T && c < Cp) reinterpret_cast<float*>(cl)[cl_at(t, c)] = tile[tx][r];
      }
    }
  } else {
    if constexpr (BF) {
      for (int i = threadIdx.x; i < kLT * kCh; i += 256) {
        const int r = i / kCh, q = i % kCh;
        const int t = t0 + r, c = c0 + 8 * q;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (t < T && c < Cp) v = *reinterpret_cast<const uint4*>(cl + cl_at(t, c) * 2);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tile[r][8 * q + 2 * e] = bf2f((uint16_t)(w[e] & 0xffffu));
          tile[r][8 * q + 2 * e + 1] = bf2f((uint16_t)(w[e] >> 16));
        }
      }
    } else {
      for (int r = ty; r < kLT; r += kStep) {
        const int t = t0 + r, c = c0 + tx;
        tile[r][tx] = (t < T && c < Cp) ? reinterpret_cast<const float*>(cl)[cl_at(t, c)] : 0.f;
      }
    }
    __syncthreads();
    for (int r = ty; r < nc; r += kStep) {
      const int c = c0 + r, t = t0 + tx;
      if (c < C && t < T) nchw[((b * C + c) * F + f) * T + t] = tile[tx][r];
    }
  }
}

}  // namespace

void launch_nchw_cl(const NchwCl& d, const ArenaBases& ab, hipStream_t st) {
  if (d.B < 1 || d.C < 1 || d.F < 1 || d.T < 1) return;
  NchwCl e = d;
  // one frame per (b, f) (ComplexBatchNorm over [B, C, S]): [B][C][F][1] is [B][C][1][F] and [B][1][F][Cpad] is [B][F][1][Cpad] - the bins take the
  // frames' place, so that the tile still covers 64 adjacent floats of the reference side
  if (e.T == 1 && e.Tcl == 1 && e.t_off == 0) { e.T = e.Tcl = d.F; e.F = 1; }
  const int64_t bf = (int64_t)e.B * e.F;
  if (bf > 65535) {                                               // grid z limit: more (b, f) pairs than one launch addresses
    // split over the batch: every launch covers whole batch items
    const int per = (int)(65535 / e.F);
    if (per < 1) return;                                          // F > 65535: refused by the planner
    for (int b0 = 0; b0 < e.B; b0 += per) {
      NchwCl p = e;
      p.B = e.B - b0 < per ? e.B - b0 : per;
      p.nchw.off += (int64_t)b0 * e.C * e.F * e.T * 4;
      p.cl.off += (int64_t)b0 * e.Tcl * e.F * e.Cpad * esize(e.dt);
      launch_nchw_cl(p, ab, st);
    }
    return;
  }
  const int lt = tune_int("LAYOUT_TILE", 64) == 32 ? 32 : 64;
  const dim3 grid((e.T + lt - 1) / lt, (e.Cpad + lt - 1) / lt, (unsigned)bf);
  if (e.dt == DT_BF16) {
    if (lt == 32) hipLaunchKernelGGL((nchw_cl_kernel<true, 32>), grid, dim3(256), 0, st, e, ab);
    else hipLaunchKernelGGL((nchw_cl_kernel<true, 64>), grid, dim3(256), 0, st, e, ab);
  } else {
    if (lt == 32) hipLaunchKernelGGL((nchw_cl_kernel<false, 32>), grid, dim3(256), 0, st, e, ab);
    else hipLaunchKernelGGL((nchw_cl_kernel<false, 64>), grid, dim3(256), 0, st, e, ab);
  }
}

}  // namespace sefd
