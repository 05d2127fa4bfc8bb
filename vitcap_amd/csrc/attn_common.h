// Internal: what the dense attention forward (attn.hip) and backward (attn_bwd.hip) share -- the packed-qkv geometry, the row-major
// swizzled LDS tile both stage their operands in and its per-lane read offsets.
#pragma once
#include "common.h"

constexpr int HD = 64;          // head dim
constexpr int NH = 12;          // heads
constexpr int QKV_LD = 2304;    // packed row: [q | k | v] x [head][64]
constexpr int KT = 64;          // keys (rows) per tile
constexpr int TILE_B = KT * 128;   // one row-major tile: 64 rows x 128 B (one row = one key's / query's 64 head dims)

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// 16-byte chunk c of LDS row r (128 B = one key's 64 head dims) is stored at chunk c ^ kv_swz(r): the 16-lane groups of the
// K fragment reads (ds_read_b128: 16 different rows, one chunk) and the 32-lane groups of the V transpose reads
// (ds_read_b64_tr_b16: 4 consecutive rows x 64 B) then touch every bank once (MI355X_MICROARCH.md, LDS).
__device__ __forceinline__ int kv_swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// Per-lane read offsets inside a tile (fixed per lane), filled into the caller's int koff_[4] and int toff_[2][2]; half_ is lane_ >> 5:
//   koff_[ds]: row-major fragment (ds_read_b128) of row lane & 31 (+32 rows: +4096), chunk (2 ds + half) ^ swz(row);
//   toff_[rd][dt]: transpose read rd of a 16-row block (block base a multiple of 16; +2048 per block) of the tile base_ bytes into the
//   stage: the lane supplies row 8 rd + 4 half + j (j = (lane & 15) >> 2), 8 bytes at dims 32 dt + 16 ((lane >> 4) & 1) + 4 (lane & 3).
// A macro, not a function: hipcc simplifies a __forceinline__ callee on its own before it inlines it, without the caller's known bits of
// `lane`, and both kernels' register allocation then comes out different (docs/LAB_refactor_kernel_switches.md).
#define ATTN_READ_OFFSETS(koff_, toff_, base_, lane_, half_)                                      \
  do {                                                                                            \
    _Pragma("unroll") for (int ds = 0; ds < 4; ++ds)                                              \
      (koff_)[ds] = ((lane_) & 31) * 128 + (((2 * ds + (half_)) ^ kv_swz((lane_) & 31)) * 16);    \
    const int j_ = ((lane_) & 15) >> 2;                                                           \
    const int c2_ = (((lane_) >> 4) & 1) * 2 + (((lane_) & 3) >> 1);                              \
    _Pragma("unroll") for (int rd = 0; rd < 2; ++rd) {                                            \
      const int r_ = 8 * rd + 4 * (half_) + j_;                                                   \
      _Pragma("unroll") for (int dt = 0; dt < 2; ++dt)                                            \
        (toff_)[rd][dt] = (base_) + r_ * 128 + (((c2_ + 4 * dt) ^ kv_swz(r_)) * 16) + ((lane_) & 1) * 8; \
    }                                                                                             \
  } while (0)
