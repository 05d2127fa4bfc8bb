// bf16 NT GEMM with fused epilogue for gfx950 (MI355X):  C = act(A . W^T + bias) (+ residual)
//
// Both operands are K-contiguous (A[M][K], W[N][K] = nn.Linear layout), which is exactly the MFMA
// fragment layout (8 consecutive k per lane), so tiles go HBM -> LDS by `global_load_lds` (16 B per
// lane, no VGPR round trip) and LDS -> VGPR by ds_read_b128.
//
// Tile: (32*WM) x (32*WN) x 64 per 256-thread workgroup (2x2 waves, each wave WM x WN MFMA tiles of
// 16x16x32).  LDS rows are 128 B (one k-tile); 16-byte chunks are XOR-swizzled with (row & 7) so the
// 16-lane ds_read_b128 groups hit 16 distinct slots.  global_load_lds writes lane-linear, hence the
// swizzle is applied on the per-lane SOURCE address and again on the read (cdna guide rule 21).
// Two LDS buffers; the next k-tile's loads are issued before the current tile's MFMAs and drained
// once per k-tile (one barrier per tile).
//
// The accumulators are computed transposed (first MFMA operand = W fragment): each lane then holds
// 4 consecutive n for one m, so bias/residual loads and the C store are 8/16-byte vectors.
#include "common.h"
#include "gemm_args.h"
#include "gemm_plan.h"

namespace {

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// wait until at most `newer` (<= K) tiles of PIECES LDS-DMA instructions each are still outstanding
template <int K, int PIECES>
__device__ __forceinline__ void wait_newer_tiles(int newer) {
  if constexpr (K <= 0) {
    wait_vmcnt<0>();
  } else {
    if (newer >= K) wait_vmcnt<(K * PIECES < 63 ? K * PIECES : 63)>();
    else wait_newer_tiles<K - 1, PIECES>(newer);
  }
}

template <int WM, int WN, int ACT, int OUT_F32, bool HAS_RES, int NST, bool ROWSTAT = false>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs p) {
  VC_LIVE_EXIT(p.live);
  constexpr int BM = 32 * WM, BN = 32 * WN, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BUF_BYTES = A_BYTES + W_BYTES;   // buffer b: A tile at b*BUF_BYTES, W tile behind it

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;

  // XCD-aware, bijective block remap: blocks that land on one XCD (id % 8) get a contiguous range of
  // tiles, n fastest, so A row-panels are shared through that XCD's L2.
  const int nwg = p.tiles_m * p.tiles_n;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tm = bid / p.tiles_n, tn = bid - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // per-lane source rows for the staging loads (row index fixed over the k loop)
  const int srow = lane >> 3;                        // 0..7 inside an 8-row glds piece
  const int schunk = (lane & 7) ^ (srow & 7);        // swizzled 16-B chunk this lane fetches
  const bf16_t* aptr[BM / 32];
  const bf16_t* wptr[BN / 32];
#pragma unroll
  for (int i = 0; i < BM / 32; ++i) {
    int r = m0 + w * (BM / 4) + i * 8 + srow;
    r = r < p.M ? r : p.M - 1;
    aptr[i] = p.A + (size_t)r * p.lda + schunk * 8;
  }
#pragma unroll
  for (int i = 0; i < BN / 32; ++i) {
    int r = n0 + w * (BN / 4) + i * 8 + srow;
    r = r < p.N ? r : p.N - 1;
    wptr[i] = p.W + (size_t)r * p.ldw + schunk * 8;
  }

  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
      glds16(aptr[i] + k0, smem + buf * BUF_BYTES + (w * (BM / 4) + i * 8) * 128);
#pragma unroll
    for (int i = 0; i < BN / 32; ++i)
      glds16(wptr[i] + k0, smem + buf * BUF_BYTES + A_BYTES + (w * (BN / 4) + i * 8) * 128);
  };

  f32x4 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;       // row inside a 16-row fragment
  const int fk = lane >> 4;         // which 8-wide k group inside a 32-wide MFMA k step
  const int nk = p.K / BK;

  // split-K (weight gradients): this workgroup owns k-tiles [t0, t1)
  int t0 = 0, t1 = nk;
  if (p.split_k > 1) {
    t0 = blockIdx.y * p.kt_per_split;
    t1 = t0 + p.kt_per_split < nk ? t0 + p.kt_per_split : nk;
  }
  // NST LDS stages, prefetch distance NST-1: the small-M (decode) shapes are LDS-DMA-latency-bound -- a 64x64 tile has
  // ~150 cycles of MFMA work per k-tile against ~800 cycles of DMA latency -- so three k-tiles are kept in flight and
  // tile t is awaited with a counted vmcnt (the newer tiles' pieces stay outstanding).
  constexpr int PIECES = BM / 32 + BN / 32;              // LDS-DMA instructions per wave per stage
#pragma unroll
  for (int i = 0; i < NST - 1; ++i)
    if (t0 + i < t1) stage(i, (t0 + i) * BK);

  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) % NST;
    // tile t has landed once at most `newer` younger tiles' pieces are outstanding (loads retire in order)
    wait_newer_tiles<NST - 2, PIECES>(t1 - 1 - t < NST - 2 ? t1 - 1 - t : NST - 2);
    // Raw s_barrier, NOT __syncthreads(): the workgroup-scope fence in __syncthreads() makes hipcc emit `s_waitcnt vmcnt(0)` in front
    // of the barrier whenever LDS-DMA is in flight -- every k-tile then waited for the YOUNGEST request and the NST-deep ring
    // degenerated to one dependent memory round trip per k-tile (seen in the ISA; the counted wait above was dead code).
    // What the barrier must order needs no fence: tile t landed for every wave (each wave's own counted vmcnt) and every wave
    // finished tile t-1, whose fragments were consumed by MFMAs behind the compiler's own lgkmcnt waits.
    __builtin_amdgcn_s_barrier();
    if (t + NST - 1 < t1) stage((t - t0 + NST - 1) % NST, (t + NST - 1) * BK);
    const char* la = smem + buf * BUF_BYTES + (wm * WM * 16 + frow) * 128;
    const char* lw = smem + buf * BUF_BYTES + A_BYTES + (wn * WN * 16 + frow) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int coff = ((ks * 4 + fk) ^ (frow & 7)) * 16;
      bf16x8 af[WM], wf[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) af[i] = *(const bf16x8*)(la + i * 16 * 128 + coff);
#pragma unroll
      for (int j = 0; j < WN; ++j) wf[j] = *(const bf16x8*)(lw + j * 16 * 128 + coff);
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: lane holds C[m][n..n+3], m = frow, n = fk*4 within each 16x16 tile
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int m = m0 + wm * WM * 16 + i * 16 + frow;
    if (m >= p.M) continue;
    int orow = m, rrow = m;
    if (p.row_group > 0) {
      const int g = m / p.row_group, in = m - g * p.row_group;
      orow = g * p.out_group_rows + p.out_row_off + in;
      rrow = p.res_periodic ? in : orow;
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = n0 + wn * WN * 16 + j * 16 + fk * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (p.split_k > 1) {
        *(f32x4*)((float*)p.C + (size_t)blockIdx.y * p.slab + (size_t)orow * p.ldc + n) = v;
        continue;
      }
      if (p.bias) {
        const f32x4 b = *(const f32x4*)(p.bias + n);
        v += b;
      }
      if (p.aux) {
        const bf16x4 za = *(const bf16x4*)(p.aux + (size_t)orow * p.ldaux + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= (float)za[e];
      }
      if (ACT == VITCAP_ACT_GELU_ERF) {
        if (p.zout) {                  // the activation's derivative at the pre-activation, for the backward's `aux`
          f32x4 d;
          v = gelu_erf4_grad(v, d);
          uint2 zo;
          zo.x = pack2bf(d[0], d[1]);
          zo.y = pack2bf(d[2], d[3]);
          *(uint2*)(p.zout + (size_t)orow * p.ldz + n) = zo;
        } else {
          v = gelu_erf4(v);
        }
      } else if (ACT == VITCAP_ACT_TANH) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
      }
      if (HAS_RES) {
        const f32x4 r = *(const f32x4*)(p.res + (size_t)rrow * p.ldr + n);
        v += r;
      }
      if (OUT_F32) {
        *(f32x4*)((float*)p.C + (size_t)orow * p.ldc + n) = v;
      } else {
        uint2 o;
        o.x = pack2bf(v[0], v[1]);
        o.y = pack2bf(v[2], v[3]);
        *(uint2*)((bf16_t*)p.C + (size_t)orow * p.ldc + n) = o;
      }
      if (ROWSTAT) acc[i][j] = v;          // keep the finished values (bias added) for the row statistics below
    }
  }
  if (ROWSTAT) {
    // Vocabulary GEMM of a decode step: next to the logits, every wave emits for each of its rows and each 32-column piece of
    // its WN*16 columns the maximum, the column of that maximum (lowest on ties, torch.argmax's rule) and sum exp(x - max) --
    // the pieces `argmax` and `log_softmax` (modeling_utils.py:846-851) are assembled from by vitcap_greedy_select_embed, and
    // the beam step's 2*beams best candidates by vitcap_row_topk_pieces, so the 30522-wide rows are never read back.
    // Piece index = first column / 32 (row stride 2*ceil(N/64) pieces whatever the tile); columns >= N never win (skipped
    // here, and the padded vocabulary columns carry a -1e30 bias).
    const int pieces = 2 * ((p.N + 63) / 64);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int m = m0 + wm * WM * 16 + i * 16 + frow;
#pragma unroll
      for (int jp = 0; jp < WN / 2; ++jp) {
        float bm = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 2 * jp; j < 2 * jp + 2; ++j) {
          const int n = n0 + wn * WN * 16 + j * 16 + fk * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = acc[i][j][e];
            if (n + e < p.N && (x > bm || (x == bm && n + e < bi))) { bm = x; bi = n + e; }
          }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {             // the row's columns are spread over the 4 lane groups fk = lane >> 4
          const float om = __shfl_xor(bm, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (om > bm || (om == bm && oi < bi)) { bm = om; bi = oi; }
        }
        float se = 0.f;
#pragma unroll
        for (int j = 2 * jp; j < 2 * jp + 2; ++j) {
          const int n = n0 + wn * WN * 16 + j * 16 + fk * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < p.N) se += expf(acc[i][j][e] - bm);
        }
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        const int piece = (n0 + wn * WN * 16 + jp * 32) >> 5;
        if (fk == 0 && m < p.M && piece < pieces)
          *(f32x4*)(p.rowstat + ((size_t)m * pieces + piece) * 4) = f32x4{bm, __int_as_float(bi), se, 0.f};
      }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// 256 x 256 x 64 kernel, 8 waves, two LDS buffers of 64 KiB, role-alternating schedule.
//
// Waves 0-3 (group A) and 4-7 (group B) sit pairwise on the four SIMDs.  Every k-tile is processed in four
// phases, one per 64x32 quadrant of the wave's 128x64 output; a phase is a LOAD segment (ds_read the
// quadrant's fragments, issue LDS-DMA for the next k-tile) followed by a COMPUTE segment (16 MFMAs under
// s_setprio 1), each closed by s_barrier.  Group B runs one barrier behind group A, so on every SIMD one
// wave is in its compute segment while its partner is in its load segment: the matrix pipe is fed by one
// wave while the other hides LDS/DMA latency (cdna guide T3/T4/T5, MI355X_MICROARCH "two waves per SIMD").
//   LDS reads complete (lgkmcnt(0)) before the barrier that ends a load segment;
//   the next k-tile's DMA is awaited (vmcnt(0)) right before the barrier after which group A reads it.
// ------------------------------------------------------------------------------------------------
// ---- LDS-free epilogue of the 256x256 kernels -------------------------------------------------------------------
// After the (operand-swapped) MFMAs a lane (frow = lane&15, fk = lane>>4) holds, for each of the wave's four 16-column
// tiles j, the 4 columns j*16 + fk*4.. of row frow.  A 4x4 transpose between the lane-group index fk and the tile index
// j -- two butterfly stages of v_permlane32_swap / v_permlane16_swap, pure VALU, no LDS round trip -- leaves the lane
// with the 16 CONSECUTIVE columns fk*16.. of its row: 4 lanes cover the wave's whole 64-column row segment (one 128-byte
// line in bf16, two in fp32) with 16-byte stores.  Replaces staging the accumulators through LDS (measured: the
// non-store part of that epilogue was ~200 us of a 1.09 ms 295424x2304x768 GEMM).
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
template <int NREG>
__device__ __forceinline__ void lane_tile_transpose(unsigned (&r)[4][NREG]) {
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const u32x2_t t = __builtin_amdgcn_permlane32_swap(r[c][k], r[c + 2][k], false, false);
      r[c][k] = t[0];
      r[c + 2][k] = t[1];
    }
#pragma unroll
  for (int c = 0; c < 4; c += 2)
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const u32x2_t t = __builtin_amdgcn_permlane16_swap(r[c][k], r[c + 1][k], false, false);
      r[c][k] = t[0];
      r[c + 1][k] = t[1];
    }
}

// acc[NI][4]: the wave's (16*NI) x 64 block (NI row tiles of 16, 4 column tiles of 16); row0/col0 = its origin in C
template <int ACT, int OUT_F32, bool HAS_RES, int NI>
__device__ __forceinline__ void epilogue_direct(f32x4 (&acc)[NI][4], const GemmArgs& p, int row0, int col0, int lane) {
  const int frow = lane & 15, fk = lane >> 4;
  f32x4 bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = col0 + j * 16 + fk * 4;
    bias4[j] = (p.bias && n < p.N) ? *(const f32x4*)(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int ncol = col0 + fk * 16;                       // first of this lane's 16 consecutive columns after the transpose
  const bool col_ok = ncol < p.N;                        // N % 16 == 0 on this path
  f32x4 rres[2][4];
#define ISSUE_RES_D(i_)                                                                                    \
  if (HAS_RES) {                                                                                           \
    const int m_ = row0 + (i_) * 16 + frow;                                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                          \
      rres[(i_) & 1][q] = (m_ < p.M && col_ok) ? *(const f32x4*)(p.res + (size_t)m_ * p.ldr + ncol + q * 4) \
                                               : f32x4{0.f, 0.f, 0.f, 0.f};                                \
  }
  ISSUE_RES_D(0);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (i + 1 < NI) { ISSUE_RES_D(i + 1); }
    const int m = row0 + i * 16 + frow;
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = acc[i][j] + bias4[j];
      if (ACT == VITCAP_ACT_GELU_ERF) {
        v[j] = gelu_erf4(v[j]);
      }
    }
    if (OUT_F32) {
      unsigned r[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) r[j][e] = __float_as_uint(v[j][e]);
      lane_tile_transpose<4>(r);
      if (m < p.M && col_ok) {
        float* dst = (float*)p.C + (size_t)m * p.ldc + ncol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 o = f32x4{__uint_as_float(r[q][0]), __uint_as_float(r[q][1]), __uint_as_float(r[q][2]), __uint_as_float(r[q][3])};
          if (HAS_RES) o += rres[i & 1][q];
          *(f32x4*)(dst + q * 4) = o;
        }
      }
    } else {
      unsigned r[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j][0] = pack2bf(v[j][0], v[j][1]);
        r[j][1] = pack2bf(v[j][2], v[j][3]);
      }
      lane_tile_transpose<2>(r);
      if (m < p.M && col_ok) {
        bf16_t* dst = (bf16_t*)p.C + (size_t)m * p.ldc + ncol;
        uint4 o0, o1;
        o0.x = r[0][0]; o0.y = r[0][1]; o0.z = r[1][0]; o0.w = r[1][1];
        o1.x = r[2][0]; o1.y = r[2][1]; o1.z = r[3][0]; o1.w = r[3][1];
        *(uint4*)dst = o0;
        *(uint4*)(dst + 8) = o1;
      }
    }
  }
#undef ISSUE_RES_D
}

// One (64*MT) x 256 output tile at (m0, n0): MT = 4 is the 256 x 256 tile; MT = 3 / 2 are the 192- / 128-row tiles a mixed
// launch uses for the rows behind the last full round of 256-row tiles (launch_256).  Same k order per output element and the
// same epilogue arithmetic whatever MT, so the results do not depend on the tile height.
// PH: build flags of the kernel -- 4 = always set, 8 = training extras (EXTRAS), 512 = in-kernel LayerNorm (LN)
template <int ACT, int OUT_F32, bool HAS_RES, int PH, int MT>
__device__ __forceinline__ void gemm256_tile(const GemmArgs& p, char* smem, const int m0, const int n0, const int cidx = 0) {
  constexpr int BK = 64;
  constexpr int A_BYTES = 256 * BK * 2, BUF_BYTES = 2 * A_BYTES;   // the W tile sits behind a full-height A slot whatever MT
  constexpr int WR = 32 * MT;                                      // rows of one wave's block (2 waves along M, 4 along N)
  constexpr int NI = 2 * MT;                                       // ... in 16-row MFMA tiles
  constexpr int NP = MT + 4;                                       // LDS-DMA pieces (8 rows x 128 B per lane group) per wave and k-tile
  constexpr bool EXTRAS = (PH & 8) != 0;   // training extras (pre-activation copy `zout`, gelu' factor `aux`) compiled in: the
                                           // inference instantiations do not carry their 32 prefetch registers (222 instead of 226 VGPRs)
  constexpr bool LN = (PH & 512) != 0;  // LayerNorm of the finished rows by the last of the row block's column tiles (GemmArgs.ln_*)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w >> 2;            // 0 = group A, 1 = group B
  const int wm = w >> 2, wn = w & 3;

  const int srow = lane >> 3;
  const int schunk = (lane & 7) ^ (srow & 7);
  const bf16_t* aptr[MT];
  const bf16_t* wptr[4];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    int r = m0 + w * (8 * MT) + i * 8 + srow;
    r = r < p.M ? r : p.M - 1;
    aptr[i] = p.A + (size_t)r * p.lda + schunk * 8;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int c = n0 + w * 32 + i * 8 + srow;
    c = c < p.N ? c : p.N - 1;
    wptr[i] = p.W + (size_t)c * p.ldw + schunk * 8;
  }
  // piece q of a k-tile: q < MT -> 8 rows of A, else 8 rows of W
#define STAGE_PIECES(q0_, q1_, buf_, k0_)                                                                          \
  _Pragma("unroll") for (int q = (q0_); q < (q1_); ++q) {                                                          \
    if (q < MT)                                                                                                    \
      glds16(aptr[q < MT ? q : 0] + (k0_), smem + (buf_) * BUF_BYTES + (w * (8 * MT) + q * 8) * 128);              \
    else                                                                                                           \
      glds16(wptr[q < MT ? 0 : q - MT] + (k0_), smem + (buf_) * BUF_BYTES + A_BYTES + (w * 32 + (q - MT) * 8) * 128); \
  }
  // DMA schedule: the pieces of k-tile t+1 are spread two per load segment over L3(t-1), L0(t), L1(t), L2(t) (slot s takes
  // pieces 2s, 2s+1; MT = 3 leaves one piece for the last slot, MT = 2 none).  Buffer (t+1)&1 is free from L3(t-1) on (its
  // last reader was L2(t-1)); the pieces must have landed before the barrier after which group A starts L0(t+1): that wait
  // is vmcnt(2) -- the two pieces of tile t+2 issued in L3(t) may stay in flight -- or vmcnt(0) when nothing newer was issued.
#define STAGE_SLOT(s_, buf_, k0_) STAGE_PIECES(2 * (s_), (2 * (s_) + 2 < NP ? 2 * (s_) + 2 : NP), buf_, k0_)

  f32x4 acc[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fk = lane >> 4;
  const int coff0 = ((0 * 4 + fk) ^ (frow & 7)) * 16;
  const int coff1 = ((1 * 4 + fk) ^ (frow & 7)) * 16;
  const int a_base = (wm * WR + frow) * 128;
  const int b_base = A_BYTES + (wn * 64 + frow) * 128;
  const int nk = p.K / BK;

  bf16x8 afr[MT][2];     // current m-half: MT m-tiles x 2 k-steps
  bf16x8 bfr[2][2][2];   // both n-halves: [nh][n-tile][k-step]

#define LOAD_A(buf_, mh_)                                                                        \
  _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                                            \
    const char* ra_ = smem + (buf_) * BUF_BYTES + a_base + ((mh_) * MT + mt) * 16 * 128;         \
    afr[mt][0] = *(const bf16x8*)(ra_ + coff0);                                                  \
    afr[mt][1] = *(const bf16x8*)(ra_ + coff1);                                                  \
  }
#define LOAD_B(buf_, nh_)                                                                        \
  _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                             \
    const char* rb_ = smem + (buf_) * BUF_BYTES + b_base + ((nh_) * 2 + nt) * 16 * 128;          \
    bfr[nh_][nt][0] = *(const bf16x8*)(rb_ + coff0);                                             \
    bfr[nh_][nt][1] = *(const bf16x8*)(rb_ + coff1);                                             \
  }
#define END_LOAD()                                          \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
  __builtin_amdgcn_sched_barrier(0);                        \
  __builtin_amdgcn_s_barrier()
#define COMPUTE(mh_, nh_)                                                                               \
  __builtin_amdgcn_s_setprio(1);                                                                        \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                      \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                   \
      _Pragma("unroll") for (int nt = 0; nt < 2; ++nt)                                                  \
        acc[(mh_) * MT + mt][(nh_) * 2 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                 \
            bfr[nh_][nt][ks], afr[mt][ks], acc[(mh_) * MT + mt][(nh_) * 2 + nt], 0, 0, 0);              \
  __builtin_amdgcn_s_setprio(0)

  // prologue: k-tile 0 into buffer 0, first two pieces of k-tile 1 into buffer 1
  STAGE_PIECES(0, NP, 0, 0);
  if (nk > 1) {
    STAGE_SLOT(0, 1, BK);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  if (grp == 1) __builtin_amdgcn_s_barrier();   // group B runs one barrier behind

  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    const bool more2 = t + 2 < nk;
    // ---- phase 0: quadrant (m-half 0, n-half 0)
    LOAD_A(buf, 0);
    LOAD_B(buf, 0);
    if (more) { STAGE_SLOT(1, buf ^ 1, (t + 1) * BK); }
    END_LOAD();
    COMPUTE(0, 0);
    __builtin_amdgcn_s_barrier();
    // ---- phase 1: (m-half 0, n-half 1)
    LOAD_B(buf, 1);
    if (more) { STAGE_SLOT(2, buf ^ 1, (t + 1) * BK); }
    END_LOAD();
    COMPUTE(0, 1);
    __builtin_amdgcn_s_barrier();
    // ---- phase 2: (m-half 1, n-half 1)
    LOAD_A(buf, 1);
    if (more) { STAGE_SLOT(3, buf ^ 1, (t + 1) * BK); }
    END_LOAD();
    COMPUTE(1, 1);
    __builtin_amdgcn_s_barrier();
    // ---- phase 3: (m-half 1, n-half 0); no LDS reads; first two pieces of k-tile t+2 (its buffer, `buf`, was last
    // read in L2 above by both groups before the barrier that precedes this segment for either group)
    if (more2) { STAGE_SLOT(0, buf, (t + 2) * BK); }
    if (grp == 1) {
      if (more2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    COMPUTE(1, 0);
    if (grp == 0) {
      if (more2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();   // match group B's extra barrier
#undef STAGE_PIECES
#undef STAGE_SLOT
#undef LOAD_A
#undef LOAD_B
#undef END_LOAD
#undef COMPUTE

  // ---- epilogue through LDS: the MFMA layout gives each lane 4 consecutive n of ONE row, i.e. 32-byte (bf16)
  // pieces of 16 different rows per store instruction; measured, that caps the output stream at ~2.2 TB/s and costs
  // 75 us per 36928x2304 GEMM.  Each wave therefore parks its accumulators (fp32) in a private (16*MT)x64 LDS patch
  // (two halves of its rows), reads them back row-major and issues full-line stores: 16 lanes cover one
  // 64-column row segment (256 B fp32 / 128 B bf16), bias / GELU / residual are applied in this coalesced pass.
  constexpr int EP_ROWB = 272;                       // 64 fp32 + 16 B pad: conflict-free ds_write_b128
  char* ep = smem + w * (64 * EP_ROWB);
  const int er = lane >> 4, ec = (lane & 15) * 4;    // read-back: row within a group of 4, first of 4 columns
  const int ncol = n0 + wn * 64 + ec;
  f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.bias && ncol < p.N) bias4 = *(const f32x4*)(p.bias + ncol);
  // residual rows are requested one chunk (2*MT iterations = 8*MT rows) ahead of their use
  const bool col_ok = ncol < p.N;
  f32x4 rres[2][2 * MT];
#define ISSUE_RES(c_)                                                                                        \
  if (HAS_RES) {                                                                                             \
    _Pragma("unroll") for (int it = 0; it < 2 * MT; ++it) {                                                  \
      const int m_ = m0 + wm * WR + (c_) * (8 * MT) + it * 4 + er;                                           \
      ROWS_OF(m_, o_, r_);                                                                                   \
      (void)o_;                                                                                              \
      rres[(c_) & 1][it] = (m_ < p.M && col_ok) ? *(const f32x4*)(p.res + (size_t)r_ * p.ldr + ncol)        \
                                                : f32x4{0.f, 0.f, 0.f, 0.f};                                 \
    }                                                                                                        \
  }
  // plain rows, no aux / pre-activation copy, bf16 output without residual or fp32 output: straight from registers
  // measured against the LDS-staged epilogue below: +4-5 % for the GELU epilogue (fc1), neutral for
  // plain bf16 (qkv), SLOWER for the fp32 + residual outputs (proj 0.078 -> 0.106 ms) -- so it is used for GELU only
  if (ACT == VITCAP_ACT_GELU_ERF && !OUT_F32 && !HAS_RES && !(EXTRAS && p.zout) && !(EXTRAS && p.aux) && p.row_group == 0 &&
      (p.N & 15) == 0 && (p.ldc & 7) == 0) {
    epilogue_direct<ACT, OUT_F32, HAS_RES, NI>(acc, p, m0 + wm * WR, n0 + wn * 64, lane);
    return;
  }
  // bf16 output, plain rows, no residual: 8 columns per lane, one 16-byte store (8 lanes = one 128-byte line of the output
  // row) -- half the store instructions of the general path below.  The training extras ride along in the same shape: the
  // pre-activation copy (zout, fc1 forward) leaves as a second 16-byte store, the gelu'(aux) factor (fc2's input gradient)
  // arrives as 16-byte loads issued for a whole half BEFORE the LDS staging, so their latency hides behind it
  // (before: 8-byte loads used immediately, scalar gelu': 337 us per call at M = 36928, N = 3072)
  if constexpr (!OUT_F32 && !HAS_RES) {
    if (p.row_group == 0 && (p.N & 7) == 0 && (p.ldc & 7) == 0 && (!(EXTRAS && p.zout) || (p.ldz & 7) == 0) && (!(EXTRAS && p.aux) || (p.ldaux & 7) == 0)) {
      const int wr = lane >> 3, wc = (lane & 7) * 8;
      const int ncw = n0 + wn * 64 + wc;
      const bool okc = ncw < p.N;
      f32x4 b_lo = f32x4{0.f, 0.f, 0.f, 0.f}, b_hi = b_lo;
      f32x4 cs_lo = f32x4{0.f, 0.f, 0.f, 0.f}, cs_hi = cs_lo;      // EXTRAS && p.colsum: this lane's 8 columns summed over its 4*MT rows
      if (p.bias && ncw < p.N) {
        b_lo = *(const f32x4*)(p.bias + ncw);
        b_hi = *(const f32x4*)(p.bias + ncw + 4);
      }
#pragma unroll
      for (int hm = 0; hm < 2; ++hm) {
        uint4 axv[2 * MT];
        if (EXTRAS && p.aux) {
#pragma unroll
          for (int it = 0; it < 2 * MT; ++it) {
            const int m = m0 + wm * WR + hm * (16 * MT) + it * 8 + wr;
            axv[it] = (m < p.M && okc) ? *(const uint4*)(p.aux + (size_t)m * p.ldaux + ncw) : uint4{0u, 0u, 0u, 0u};
          }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            *(f32x4*)(ep + (i * 16 + frow) * EP_ROWB + (j * 16 + fk * 4) * 4) = acc[hm * MT + i][j];
#pragma unroll
        for (int it = 0; it < 2 * MT; ++it) {
          const int rl = it * 8 + wr;
          f32x4 v0 = *(const f32x4*)(ep + rl * EP_ROWB + wc * 4);
          f32x4 v1 = *(const f32x4*)(ep + rl * EP_ROWB + wc * 4 + 16);
          const int m = m0 + wm * WR + hm * (16 * MT) + rl;
          const bool ok = m < p.M && okc;
          v0 += b_lo;
          v1 += b_hi;
          if (EXTRAS && p.aux) {
            const uint4 a = axv[it];
            v0 *= f32x4{__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xffff0000u), __uint_as_float(a.y << 16),
                        __uint_as_float(a.y & 0xffff0000u)};
            v1 *= f32x4{__uint_as_float(a.z << 16), __uint_as_float(a.z & 0xffff0000u), __uint_as_float(a.w << 16),
                        __uint_as_float(a.w & 0xffff0000u)};
          }
          if (ACT == VITCAP_ACT_GELU_ERF) {
            if (EXTRAS && p.zout) {      // gelu'(pre-activation) from the same erfc evaluation, for the backward's `aux`
              f32x4 d0, d1;
              v0 = gelu_erf4_grad(v0, d0);
              v1 = gelu_erf4_grad(v1, d1);
              if (ok) {
                uint4 zo;
                zo.x = pack2bf(d0[0], d0[1]);
                zo.y = pack2bf(d0[2], d0[3]);
                zo.z = pack2bf(d1[0], d1[1]);
                zo.w = pack2bf(d1[2], d1[3]);
                *(uint4*)(p.zout + (size_t)m * p.ldz + ncw) = zo;
              }
            } else {
              v0 = gelu_erf4(v0);
              v1 = gelu_erf4(v1);
            }
          }
          if (ok) {
            uint4 o;
            o.x = pack2bf(v0[0], v0[1]);
            o.y = pack2bf(v0[2], v0[3]);
            o.z = pack2bf(v1[0], v1[1]);
            o.w = pack2bf(v1[2], v1[3]);
            *(uint4*)((bf16_t*)p.C + (size_t)m * p.ldc + ncw) = o;
            if (EXTRAS && p.colsum) {         // the ROUNDED values, as vitcap_colsum_bf16 over the stored output would add them
              cs_lo += f32x4{__uint_as_float(o.x << 16), __uint_as_float(o.x & 0xffff0000u), __uint_as_float(o.y << 16),
                             __uint_as_float(o.y & 0xffff0000u)};
              cs_hi += f32x4{__uint_as_float(o.z << 16), __uint_as_float(o.z & 0xffff0000u), __uint_as_float(o.w << 16),
                             __uint_as_float(o.w & 0xffff0000u)};
            }
          }
        }
      }
      if (EXTRAS && p.colsum) {
        // the 8 lanes wr = 0..7 with the same (lane & 7) hold the same 8 columns: butterfly over lane bits 3..5, then one atomic
        // per column and wave (two waves of the workgroup share each column: 512 atomics per 256x256 tile)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int o = 8; o <= 32; o <<= 1) {
            cs_lo[e] += __shfl_xor(cs_lo[e], o, 64);
            cs_hi[e] += __shfl_xor(cs_hi[e], o, 64);
          }
        }
        if (wr == 0 && okc) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            atomicAdd(p.colsum + ncw + e, cs_lo[e]);
            atomicAdd(p.colsum + ncw + 4 + e, cs_hi[e]);
          }
        }
      }
      return;
    }
  }
  // fused LayerNorm launches address C through a buffer descriptor from the tile's first row (plain rows only)
  const __amdgpu_buffer_rsrc_t ln_rc = vc_rsrc(LN ? (const char*)p.C + (size_t)m0 * p.ldc * 4 : nullptr, LN ? (long long)(p.M - m0) * p.ldc * 4 : 0);
  ISSUE_RES(0);
#pragma unroll
  for (int hm = 0; hm < 2; ++hm) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *(f32x4*)(ep + (i * 16 + frow) * EP_ROWB + (j * 16 + fk * 4) * 4) = acc[hm * MT + i][j];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int c = hm * 2 + ch;
      if (c + 1 < 4) { ISSUE_RES(c + 1); }
#pragma unroll
      for (int it = 0; it < 2 * MT; ++it) {
        const int rl = ch * (8 * MT) + it * 4 + er;
        f32x4 v = *(const f32x4*)(ep + rl * EP_ROWB + ec * 4);
        const int m = m0 + wm * WR + hm * (16 * MT) + rl;
        const bool ok = m < p.M && col_ok;
        ROWS_OF(m, orow, rrow);
        (void)rrow;
        v += bias4;
        if (EXTRAS && p.aux && ok) {
          const bf16x4 za = *(const bf16x4*)(p.aux + (size_t)orow * p.ldaux + ncol);
          v *= f32x4{(float)za[0], (float)za[1], (float)za[2], (float)za[3]};
        }
        if (ACT == VITCAP_ACT_GELU_ERF) {
          if (EXTRAS && p.zout) {
            f32x4 d;
            v = gelu_erf4_grad(v, d);
            if (ok) {
              uint2 zo;
              zo.x = pack2bf(d[0], d[1]);
              zo.y = pack2bf(d[2], d[3]);
              *(uint2*)(p.zout + (size_t)orow * p.ldz + ncol) = zo;
            }
          } else {
            v = gelu_erf4(v);
          }
        }
        if (HAS_RES) v += rres[c & 1][it];
        if (ok) {
          if (OUT_F32) {
            if constexpr (LN) {
              // write-through (sc1): the row block's last-arriving workgroup reads these rows back, wherever on the chip it runs
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vc_u32x4, v), ln_rc, (unsigned)((orow - m0) * p.ldc + ncol) * 4u, 0, 16);
            } else {
              *(f32x4*)((float*)p.C + (size_t)orow * p.ldc + ncol) = v;
            }
          } else {
            uint2 o;
            o.x = pack2bf(v[0], v[1]);
            o.y = pack2bf(v[2], v[3]);
            *(uint2*)((bf16_t*)p.C + (size_t)orow * p.ldc + ncol) = o;
          }
        }
      }
    }
  }
#undef ISSUE_RES
  if constexpr (LN) {
    // ---- LayerNorm of the row block by the LAST of its column tiles to get here (any placement of the tiles over XCDs / CUs):
    // every wave's write-through stores acknowledged -> barrier -> one relaxed agent-scope ticket; the workgroup that draws the last
    // ticket reads the block's rows back with sc1 loads (they bypass this CU's L1 and the XCD's L2 lines other XCDs wrote behind)
    // and normalises them with the LayerNorm kernel's own row function.  The ticket counter goes back to zero for the next launch.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* s_flag = (int*)smem;
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(p.ln_cnt + cidx, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == p.tiles_n - 1;
      if (last) __hip_atomic_store(p.ln_cnt + cidx, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *s_flag = last;
    }
    __syncthreads();
    if (*s_flag == 0) return;
    if (!p.ln_out && !p.ln_out_f) return;      // (timing experiments: publish only)
    // the other tiles' rows sit in memory (write-through); one agent-scope acquire drops whatever this CU's L1 holds of them, then
    // plain loads fetch them through the L2 at the ordinary rate (sc1 loads measured 5x slower here: 85 row blocks finish together
    // and the uncached path serves them one after the other)
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
    const int rows = p.M - m0 < 64 * MT ? p.M - m0 : 64 * MT;
    constexpr int RB = 8;                      // rows in flight per wave: 8 waves x 8 rows x 3 KB = 196 KB of requests per pass
    for (int r0 = w * RB; r0 < rows; r0 += 8 * RB) {
      f32x4 v[RB][3];
#pragma unroll
      for (int j = 0; j < RB; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i)           // rows past the block's end: the descriptor's range check returns zeros for the last block only
          v[j][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ln_rc, (unsigned)((r0 + j) * p.ldc + i * 256 + lane * 4) * 4u, 0, 0));
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const int row = m0 + r0 + j;
        if (r0 + j < rows)
          ln_row(v[j], p.ln_g, p.ln_b, p.ln_eps, lane, p.ln_out ? p.ln_out + (size_t)row * D768 : nullptr,
                 p.ln_out_f ? p.ln_out_f + (size_t)row * D768 : nullptr);
      }
    }
  }
}

// The launch: n_big workgroups own 256-row tiles of rows [0, 256 * tiles_m); with MTS != 0 the workgroups behind them own
// (64*MTS)-row tiles of the remaining rows.  Workgroups are dispatched in blockIdx order (block b on XCD b % 8), so every XCD
// works through its share of the big tiles first and fills the last, partial round with the short ones.
// VGPR cap 224: two waves of this kernel per SIMD then leave 64 of the 512 registers (and 24 KB of LDS) free, which is what one wave
// of the decode step's HBM-bound attention kernel needs (60 VGPRs, 8 KB): in the 2-slot batch pipeline that kernel can become
// RESIDENT NEXT TO the GEMM's workgroups instead of waiting for CUs to drain -- K/V streaming overlaps the MFMA work.
#define VC_GEMM256_VGPRS 224
template <int ACT, int OUT_F32, bool HAS_RES, int PH, int MTS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(VC_GEMM256_VGPRS))) void gemm_nt_256_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bid = blockIdx.x;
  const bool small = MTS != 0 && bid >= p.n_big;
  if (small) bid -= p.n_big;       // the XCD of block b is b % 8: subtracting a constant rotates the XCD ids, chunks stay whole
  const int tiles_m = small ? p.tiles_m_small : p.tiles_m;
  {
    // XCD-aware, bijective remap: the blocks of one XCD get a contiguous chunk of the region's tile list
    const int nwg = tiles_m * p.tiles_n;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  // column groups of group_n tiles: the tiles an XCD runs at once are consecutive positions of its chunk, so they span few W
  // tiles (which stay in its L2 for the walk down M) and each A tile is fetched once for group_n consumers
  const int per_g = tiles_m * p.group_n;
  const int gi = bid / per_g, rem = bid - gi * per_g;
  const int gleft = p.tiles_n - gi * p.group_n;
  const int gw = gleft < p.group_n ? gleft : p.group_n;
  int tm = rem / gw;
  const int tn = gi * p.group_n + rem - tm * gw;
  // walk direction (call_state.h: vc_tls_walk_rev): row tiles last-to-first, and every other column group the other way round (a
  // group's pass over A ends where the next one starts)
  if ((p.rev != 0) != ((gi & 1) != 0)) tm = tiles_m - 1 - tm;
  if (!small) {
    gemm256_tile<ACT, OUT_F32, HAS_RES, PH, 4>(p, smem, tm * 256, tn * 256, tm);
  } else {
    if constexpr (MTS != 0) gemm256_tile<ACT, OUT_F32, HAS_RES, PH, MTS>(p, smem, p.tiles_m * 256 + tm * (64 * MTS), tn * 256, p.tiles_m + tm);
  }
}

template <int ACT, int OUT_F32, bool HAS_RES, int PH, int MTS>
int launch_256_t(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  auto kern = gemm_nt_256_kernel<ACT, OUT_F32, HAS_RES, PH, MTS>;
  VC_FUNC_SMEM(kern, pl.lds_bytes);
  VC_LAUNCH_GEMM(kern, dim3(pl.grid[0]), dim3(512), pl.lds_bytes, s, p);
  VC_LAUNCH_CHECK("gemm_nt_256");
  return VITCAP_OK;
}

// the plan's (ph, mts) onto the builds: training extras and fused LayerNorm run 256-row tiles only (gemm_plan.cpp: plan_8w)
template <int ACT, int OUT_F32, bool HAS_RES>
int launch_256(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  if (pl.ph == (4 | 8)) return launch_256_t<ACT, OUT_F32, HAS_RES, 4 | 8, 0>(p, pl, s);
  if (pl.mts == 3) return launch_256_t<ACT, OUT_F32, HAS_RES, 4, 3>(p, pl, s);
  if (pl.mts == 2) return launch_256_t<ACT, OUT_F32, HAS_RES, 4, 2>(p, pl, s);
  return launch_256_t<ACT, OUT_F32, HAS_RES, 4, 0>(p, pl, s);
}

int dispatch_256(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  if (pl.ln_fused)
    return pl.has_res ? launch_256_t<VITCAP_ACT_NONE, 1, true, 4 | 512, 0>(p, pl, s) : launch_256_t<VITCAP_ACT_NONE, 1, false, 4 | 512, 0>(p, pl, s);
#define CASE(ACT_, OUT_)                        \
  if (pl.act == ACT_ && pl.out_f32 == OUT_)     \
    return pl.has_res ? launch_256<ACT_, OUT_, true>(p, pl, s) : launch_256<ACT_, OUT_, false>(p, pl, s);
  CASE(VITCAP_ACT_NONE, 0)
  CASE(VITCAP_ACT_NONE, 1)
  CASE(VITCAP_ACT_GELU_ERF, 0)
  CASE(VITCAP_ACT_GELU_ERF, 1)
#undef CASE
  vitcap_set_error("gemm(256): no build for act %d / out %d", pl.act, pl.out_f32);
  return VITCAP_EINVAL;
}


// ------------------------------------------------------------------------------------------------
// Skinny kernel for the decode-step GEMMs (M = 2B or B rows: 64..256).  These are weight-streaming,
// latency-bound problems: the whole weight matrix is read once and there is almost no reuse, so LDS
// staging buys nothing (cdna guide "GEMV / M <= 16 decode weights ... load straight to VGPRs, deep
// unroll, late vmcnt").  Each wave owns a 32x32 output patch and loads its MFMA fragments directly
// from global memory (16 B per lane, the fragment layout IS the memory layout for K-contiguous
// operands); two register sets of 4 k-steps (128 k) each keep 16 loads in flight while the other set
// is multiplied.  Parallelism comes from narrow 32-column tiles and split-K: with split_k > 1 the
// kernel writes fp32 partial slabs P[kz][M][N] and the consumer (vitcap_sum_layernorm) reduces them.
// ------------------------------------------------------------------------------------------------
struct SkinnyArgs {
  GemmArgs g;
  int split_k;     // >= 1
  int kc;          // k range per split (multiple of 128)
  size_t slab;     // elements between partial slabs
};

template <int WAVES_M, int ACT, int OUT_F32, bool HAS_RES, bool PARTIAL>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(SkinnyArgs q) {
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int BM = 32 * WAVES_M, BN = 32 * WAVES_N;
  const GemmArgs& p = q.g;
  VC_LIVE_EXIT(p.live);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w / WAVES_N, wn = w % WAVES_N;
  const int n0 = blockIdx.x * BN + wn * 32;
  const int m0 = blockIdx.y * BM + wm * 32;
  const int kz = blockIdx.z;
  const int kbeg = kz * q.kc;
  const int frow = lane & 15, fk = lane >> 4;

  const bf16_t* ap[2];
  const bf16_t* wp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int r = m0 + i * 16 + frow;
    r = r < p.M ? r : p.M - 1;
    ap[i] = p.A + (size_t)r * p.lda + kbeg + fk * 8;
    int c = n0 + i * 16 + frow;
    c = c < p.N ? c : p.N - 1;
    wp[i] = p.W + (size_t)c * p.ldw + kbeg + fk * 8;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 a0[4][2], w0[4][2], a1[4][2], w1[4][2];
#define LOADSET(A_, W_, k0_)                                                   \
  _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                           \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                         \
      A_[s_][i_] = *(const bf16x8*)(ap[i_] + (k0_) + s_ * 32);                 \
      W_[s_][i_] = *(const bf16x8*)(wp[i_] + (k0_) + s_ * 32);                 \
    }                                                                          \
  }
#define MMASET(A_, W_)                                                                          \
  _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_)                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                            \
      _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                          \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W_[s_][j_], A_[s_][i_], acc[i_][j_], 0, 0, 0);

  const int nch = q.kc / 128;
  LOADSET(a0, w0, 0);
  for (int c = 0; c < nch; c += 2) {
    if (c + 1 < nch) { LOADSET(a1, w1, (c + 1) * 128); }
    MMASET(a0, w0);
    if (c + 1 < nch) {
      if (c + 2 < nch) { LOADSET(a0, w0, (c + 2) * 128); }
      MMASET(a1, w1);
    }
  }
#undef LOADSET
#undef MMASET

#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + i * 16 + frow;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + j * 16 + fk * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (PARTIAL) {
        *(f32x4*)((float*)p.C + (size_t)kz * q.slab + (size_t)m * p.ldc + n) = v;
        continue;
      }
      if (p.bias) v += *(const f32x4*)(p.bias + n);
      if (ACT == VITCAP_ACT_GELU_ERF) {
        v = gelu_erf4(v);
      } else if (ACT == VITCAP_ACT_TANH) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
      }
      if (HAS_RES) v += *(const f32x4*)(p.res + (size_t)m * p.ldr + n);
      if (OUT_F32) {
        *(f32x4*)((float*)p.C + (size_t)m * p.ldc + n) = v;
      } else {
        uint2 o;
        o.x = pack2bf(v[0], v[1]);
        o.y = pack2bf(v[2], v[3]);
        *(uint2*)((bf16_t*)p.C + (size_t)m * p.ldc + n) = o;
      }
    }
  }
}

// ---- launchers: they take what the plan says (gemm_plan.cpp) and decide nothing ----------------------------------------------------
template <int WAVES_M>
int launch_skinny(const GemmArgs& a, const GemmPlan& pl, hipStream_t s) {
  SkinnyArgs q;
  q.g = a;
  q.split_k = pl.split_k;
  q.kc = pl.kt_per_split * 64;
  q.slab = (size_t)pl.slab;
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]);
#define SK(ACT_, OUT_, RES_, PART_)                                                                 \
  if (pl.act == ACT_ && pl.out_f32 == OUT_ && (pl.has_res != 0) == RES_ && (pl.partial != 0) == PART_) \
    hipLaunchKernelGGL((gemm_skinny_kernel<WAVES_M, ACT_, OUT_, RES_, PART_>), grid, dim3(256), 0, s, q)
  SK(0, 1, false, true);
  SK(0, 0, false, false);
  SK(0, 1, false, false);
  SK(0, 1, true, false);
  SK(0, 0, true, false);
  SK(1, 0, false, false);
  SK(1, 1, false, false);
  SK(2, 0, false, false);
  SK(2, 1, false, false);
#undef SK
  VC_LAUNCH_CHECK("gemm_skinny");
  return VITCAP_OK;
}

// gemm_nt_kernel, every family (ring / resident / rowstat): one instantiation of this launcher per kernel, so VC_FUNC_SMEM's
// per-call-site memory is per kernel.  The ring's tiles of up to 48 KiB need no attribute
template <int WM, int WN, int ACT, int OUT_F32, bool HAS_RES, int NST, bool ROWSTAT = false>
int launch_nt(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  auto kern = gemm_nt_kernel<WM, WN, ACT, OUT_F32, HAS_RES, NST, ROWSTAT>;
  if (pl.family != VITCAP_GEMM_FAMILY_RING || pl.lds_bytes > 48 * 1024) VC_FUNC_SMEM(kern, pl.lds_bytes);
  hipLaunchKernelGGL(kern, dim3(pl.grid[0], pl.grid[1]), dim3(256), pl.lds_bytes, s, p);
  VC_LAUNCH_CHECK(ROWSTAT ? "gemm_nt(rowstat)" : NST == 12 ? "gemm_nt(resident)" : "gemm_nt");
  return VITCAP_OK;
}

// "Resident" form (12 stages = the whole 768-long k range of the workgroup in LDS: 12 * (BM + BN) * 128 B <= 160 KiB, BM + BN <= 96)
template <int WM, int WN>
int dispatch_resident(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  static_assert(12 * (32 * WM + 32 * WN) * 64 * 2 <= 160 * 1024, "resident tile does not fit the LDS");
  const int act = pl.act, out = pl.out_f32, res = pl.has_res;
  if (act == VITCAP_ACT_NONE && !out && !res) return launch_nt<WM, WN, VITCAP_ACT_NONE, 0, false, 12>(p, pl, s);
  if (act == VITCAP_ACT_NONE && out && !res) return launch_nt<WM, WN, VITCAP_ACT_NONE, 1, false, 12>(p, pl, s);
  if (act == VITCAP_ACT_NONE && out && res) return launch_nt<WM, WN, VITCAP_ACT_NONE, 1, true, 12>(p, pl, s);
  if (act == VITCAP_ACT_GELU_ERF && !out && !res) return launch_nt<WM, WN, VITCAP_ACT_GELU_ERF, 0, false, 12>(p, pl, s);
  if (act == VITCAP_ACT_GELU_ERF && out && !res) return launch_nt<WM, WN, VITCAP_ACT_GELU_ERF, 1, false, 12>(p, pl, s);
  vitcap_set_error("gemm(resident): no build for act=%d out=%d res=%d", act, out, res);
  return VITCAP_EINVAL;
}

// LDS-staged ring: small tiles (decode shapes) 4 stages, 128x128 tiles 2 (gemm_plan.cpp: plan_ring)
template <int WM, int WN>
int dispatch(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  constexpr int NST = (WM <= 2 && WN <= 2) ? 4 : 2;
#define CASE(ACT_, OUT_)                                                         \
  if (pl.act == ACT_ && pl.out_f32 == OUT_)                                      \
    return pl.has_res ? launch_nt<WM, WN, ACT_, OUT_, true, NST>(p, pl, s) : launch_nt<WM, WN, ACT_, OUT_, false, NST>(p, pl, s);
  CASE(VITCAP_ACT_NONE, 0)
  CASE(VITCAP_ACT_NONE, 1)
  CASE(VITCAP_ACT_GELU_ERF, 0)
  CASE(VITCAP_ACT_GELU_ERF, 1)
  CASE(VITCAP_ACT_TANH, 0)
  CASE(VITCAP_ACT_TANH, 1)
#undef CASE
  vitcap_set_error("gemm: no build for act %d / out %d", pl.act, pl.out_f32);
  return VITCAP_EINVAL;
}

// the one switch from the plan onto the template launchers
int launch_plan(const GemmArgs& p, const GemmPlan& pl, hipStream_t s) {
  const int tile = pl.wm * 10 + pl.wn;
  switch (pl.family) {
    case VITCAP_GEMM_FAMILY_RING:
      if (tile == 11) return dispatch<1, 1>(p, pl, s);
      if (tile == 12) return dispatch<1, 2>(p, pl, s);
      if (tile == 21) return dispatch<2, 1>(p, pl, s);
      if (tile == 22) return dispatch<2, 2>(p, pl, s);
      if (tile == 44) return dispatch<4, 4>(p, pl, s);
      break;
    case VITCAP_GEMM_FAMILY_RESIDENT:
      if (tile == 21) return dispatch_resident<2, 1>(p, pl, s);
      if (tile == 11) return dispatch_resident<1, 1>(p, pl, s);
      if (tile == 12) return dispatch_resident<1, 2>(p, pl, s);
      break;
    case VITCAP_GEMM_FAMILY_ROWSTAT:
      if (tile == 22) return launch_nt<2, 2, VITCAP_ACT_NONE, 1, false, 4, true>(p, pl, s);
      if (tile == 44) return launch_nt<4, 4, VITCAP_ACT_NONE, 1, false, 2, true>(p, pl, s);
      break;
    case VITCAP_GEMM_FAMILY_SKINNY:
      return pl.wm == 2 ? launch_skinny<2>(p, pl, s) : launch_skinny<4>(p, pl, s);
    case VITCAP_GEMM_FAMILY_8WAVE:
      return dispatch_256(p, pl, s);
    case VITCAP_GEMM_FAMILY_4WAVE_TILE:
    case VITCAP_GEMM_FAMILY_4WAVE_PERSISTENT:
      return vc_launch_4w(p, pl, s);
  }
  vitcap_set_error("gemm: no launcher for family %d, tile %d x %d waves", pl.family, pl.wm, pl.wn);
  return VITCAP_EINVAL;
}

}  // namespace

extern "C" int vitcap_gemm_bias_act(const void* A, const void* W, const float* bias, const float* residual,
                                    void* C, const vitcap_gemm_desc* d, void* stream) {
  return vitcap_gemm_ex(A, W, bias, residual, C, d, nullptr, 0, nullptr, 0, stream);
}

extern "C" int vitcap_gemm_ex(const void* A, const void* W, const float* bias, const float* residual, void* C,
                              const vitcap_gemm_desc* d, const void* aux_bf16, int ldaux, void* zout_bf16, int ldz,
                              void* stream) {
  VC_REQUIRE(A && W && C && d, "gemm: null pointer");
  // every other check and the whole choice of the launch form: the plan (the pointer VALUES only enter as alignment bits)
  const auto off16 = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
  const unsigned misaligned = (off16(A) || off16(W) || off16(C) ? 1u : 0u) | (off16(residual) ? 2u : 0u) | (off16(bias) ? 4u : 0u);
  GemmPlan pl;
  const int rc = vc_gemm_plan(d, GemmOperands{bias != nullptr, residual != nullptr, aux_bf16 != nullptr, zout_bf16 != nullptr, ldaux, ldz, misaligned}, &pl);
  if (rc != VITCAP_OK) return rc;
  GemmArgs a;
  a.A = (const bf16_t*)A;
  a.W = (const bf16_t*)W;
  a.bias = bias;
  a.res = residual;
  a.C = C;
  a.M = d->M; a.N = d->N; a.K = d->K;
  a.lda = d->lda; a.ldw = d->ldw; a.ldc = d->ldc; a.ldr = d->ldr;
  a.row_group = d->row_group; a.out_group_rows = d->out_group_rows;
  a.out_row_off = d->out_row_off; a.res_periodic = d->res_periodic;
  a.tiles_m = pl.tiles_m; a.tiles_n = pl.tiles_n;
  a.n_big = pl.n_big; a.tiles_m_small = pl.tiles_m_small; a.group_n = pl.group_n;
  a.aux = (const bf16_t*)aux_bf16; a.ldaux = ldaux;
  a.colsum = d->colsum;
  a.zout = (bf16_t*)zout_bf16; a.ldz = ldz;
  a.split_k = 1; a.kt_per_split = 0; a.slab = 0;
  if (pl.family != VITCAP_GEMM_FAMILY_SKINNY) {      // the skinny kernel takes its splits beside the block (SkinnyArgs)
    a.split_k = pl.split_k; a.kt_per_split = pl.kt_per_split; a.slab = (size_t)pl.slab;
  }
  a.live = d->live;
  a.rev = vc_tls_walk_rev ? 1 : 0;
  a.rowstat = (float*)d->rowstat;
  a.ln_g = a.ln_b = nullptr; a.ln_eps = 0.f; a.ln_out = nullptr; a.ln_out_f = nullptr; a.ln_cnt = nullptr;
  if (pl.ln_fused) {
    a.ln_g = d->ln_gamma; a.ln_b = d->ln_beta; a.ln_eps = d->ln_eps;
    a.ln_out = (bf16_t*)d->ln_out_bf16; a.ln_out_f = d->ln_out_f32; a.ln_cnt = d->ln_counters;
  }
  const int rc1 = launch_plan(a, pl, (hipStream_t)stream);
  if (rc1 != VITCAP_OK || !pl.ln_follows) return rc1;
  // the LayerNorm reads the rows the GEMM has just written: it walks them the other way round (call_state.h: vc_tls_walk_rev; only the
  // engine ever sets the flag, and only there does this flip have an effect worth having)
  const bool dir = vc_tls_walk_rev;
  if (vc_tls_zigzag && d->M >= 2048) vc_tls_walk_rev = !dir;
  const int rc2 = vitcap_layernorm_fwd((const float*)C, d->ldc, d->ln_gamma, d->ln_beta, d->ln_eps, d->ln_out_bf16, d->ln_out_f32, d->M, 768, stream);
  vc_tls_walk_rev = dir;
  return rc2;
}
