// Text-grid attention of the one-pass caption scorer (vitcap_attn_text_grid, include/vitcap_hip.h).
//
// Every token of a scored caption is known in advance, so the 19 decode steps collapse into one grid of R = 2 * L - 1 rows per
// caption: rows 0..L-1 the tokens at positions 0..L-1, row L + j the [MASK] probe at position j + 1 -- the rows
// vitcap_embed_rows(rows_per_seq = R, pos_wrap = L) writes.  Mask (modeling_bert.py:846-876 for all steps at once): token row r
// attends the image's 578 visual rows and token rows <= r; probe j attends the visual rows, token rows 0..j and itself.
//
// One workgroup (4 waves) per (head, image, group of <= GRID_G captions of that image), following attn_decode_beam_kernel:
//   * the image's visual K rows and its V^T panel (vitcap_attn_beam_vt) are loaded into registers ONCE per workgroup (wave w owns the
//     16-key score blocks w, w + 4, .. and the 32-key P.V blocks w, w + 4, ..) and reused by every query tile of every caption;
//   * a query tile = 16 rows of one caption = the 16 columns of mfma_f32_16x16x32_bf16;
//   * the caption's own <= 79 rows are five more masked 16-key score blocks and three more 32-key P.V blocks, their V read from a
//     transposed copy staged in LDS once per caption.
// Softmax exactly as the decode kernels: raw scores staged in LDS, m = ceil(max * c), P = exp2(s * c - m) rounded to bf16 for the
// product, row sum from the unrounded P; the four waves' partial sums are added in wave order.
#include "attn_common.h"

namespace {

constexpr int VT_KP = 608;              // visual keys of the V^T panel (578 padded with zeros), as attn.hip
constexpr int GRID_S = 578;             // visual rows per image
constexpr int GRID_TK = 96;             // a caption's text keys, padded to three 32-key blocks (R <= 79)
constexpr int GRID_SC_LD = VT_KP + GRID_TK + 1;      // 705 fp32 scores per query row (odd: rows start in different LDS banks)
constexpr int GRID_VT_LD = GRID_TK + 8; // bf16 per row of the staged text V^T (208 B: 16-byte aligned, rows spread over the banks)
constexpr int GRID_G = 8;               // captions per workgroup
constexpr int GRID_NKB = (GRID_S + 15) / 16;         // 37 visual score blocks
constexpr int GRID_MAXB = (GRID_NKB + 3) / 4;        // 10 per wave
constexpr int GRID_NVB = VT_KP / 32;                 // 19 visual P.V blocks
constexpr int GRID_MAXV = (GRID_NVB + 3) / 4;        // 5 per wave
constexpr int GRID_MW = VT_KP / 32;                  // 19 mask words per caption (vitcap_attn_text_grid_masked)
constexpr size_t GRID_SMEM = (size_t)16 * GRID_SC_LD * 4 + (size_t)4 * 16 * HD * 4 + (size_t)HD * GRID_VT_LD * 2;   // 74 816 B

// MASKED (vitcap_attn_text_grid_masked): vis_mask holds GRID_MW words per caption, bit k & 31 of word k >> 5 set = visual key k is
// visible to every row of that caption; a hidden key scores -inf before the row maximum is taken.  Token keys and the probe's own key
// are never masked, so no row is empty.  The word of a 16-key score block is wave-uniform: one scalar load per block.
template <bool MASKED>
__global__ __launch_bounds__(256) void attn_text_grid_kernel(const bf16_t* __restrict__ qkv_text, const bf16_t* __restrict__ vis_qkv,
                                                             const bf16_t* __restrict__ vis_vt, bf16_t* __restrict__ out,
                                                             const uint32_t* __restrict__ vis_mask, int caps_per_image,
                                                             int groups_per_image, int L, float c_log2) {
  extern __shared__ __attribute__((aligned(16))) char grid_smem[];
  float (*sc)[GRID_SC_LD] = (float (*)[GRID_SC_LD])grid_smem;                                     // [16][705]
  float (*s_o)[HD] = (float (*)[HD])(grid_smem + (size_t)16 * GRID_SC_LD * 4);                    // [4 * 16][64]: wave w, query q -> row w * 16 + q
  bf16_t (*s_vt)[GRID_VT_LD] = (bf16_t (*)[GRID_VT_LD])(grid_smem + (size_t)16 * GRID_SC_LD * 4 + (size_t)4 * 16 * HD * 4);   // [64][104]
  __shared__ float s_max[16][4];
  __shared__ float s_l[16][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = blockIdx.x, img = blockIdx.y / groups_per_image, g = blockIdx.y - img * groups_per_image;
  const int frow = lane & 15, fk = lane >> 4;
  const int R = 2 * L - 1;
  const int c0 = g * GRID_G;
  const int ncap = caps_per_image - c0 < GRID_G ? caps_per_image - c0 : GRID_G;
  const int ntile = (R + 15) >> 4;            // query tiles = 16-key text score blocks (<= 5)

  // the image's visual K fragments and V^T fragments, requested once for the whole workgroup
  bf16x8 kf[GRID_MAXB][2];
#pragma unroll
  for (int i = 0; i < GRID_MAXB; ++i) {
    const int kb = w + 4 * i;
    if (kb < GRID_NKB) {
      int key = kb * 16 + frow;
      key = key < GRID_S ? key : GRID_S - 1;
      const bf16_t* kp = vis_qkv + ((size_t)img * GRID_S + key) * QKV_LD + 768 + h * HD + fk * 8;
      kf[i][0] = *(const bf16x8*)kp;
      kf[i][1] = *(const bf16x8*)(kp + 32);
    }
  }
  bf16x8 vf[GRID_MAXV][4];
  const bf16_t* vtb = vis_vt + ((size_t)img * NH + h) * HD * VT_KP;
#pragma unroll
  for (int i = 0; i < GRID_MAXV; ++i) {
    const int kb = w + 4 * i;
    if (kb < GRID_NVB) {
#pragma unroll
      for (int db = 0; db < 4; ++db) vf[i][db] = *(const bf16x8*)(vtb + (size_t)(db * 16 + frow) * VT_KP + kb * 32 + fk * 8);
    }
  }
  // score columns nobody writes again: the padded visual keys 592..607 and the text keys past the last text score block
  for (int i = tid; i < 16 * (16 + GRID_TK); i += 256) {
    const int q = i / (16 + GRID_TK), k = i - q * (16 + GRID_TK);
    const int col = k < 16 ? GRID_NKB * 16 + k : VT_KP + (k - 16);
    if (k < 16 || k - 16 >= ntile * 16) sc[q][col] = -INFINITY;
  }

  for (int c = 0; c < ncap; ++c) {
    const size_t cap = (size_t)img * caps_per_image + c0 + c;
    const bf16_t* rows = qkv_text + cap * R * QKV_LD + h * HD;      // row r of this caption, head h: rows + r * QKV_LD (+768 K, +1536 V)
    // the caption's V rows, transposed into LDS: s_vt[d][key], zeros behind row R-1 (every wave has left the previous caption's P.V:
    // the barrier that follows its last tile)
    for (int i = tid; i < GRID_TK * 8; i += 256) {
      const int key = i >> 3, sub = i & 7;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (key < R) v = *(const uint4*)(rows + (size_t)key * QKV_LD + 1536 + sub * 8);
      const bf16_t* e = (const bf16_t*)&v;
#pragma unroll
      for (int j = 0; j < 8; ++j) s_vt[sub * 8 + j][key] = e[j];
    }
    // the caption's K fragments: wave w owns text score blocks w and w + 4
    bf16x8 tkf[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int kb = w + 4 * i;
      if (kb < ntile) {
        int key = kb * 16 + frow;
        key = key < R ? key : R - 1;
        const bf16_t* kp = rows + (size_t)key * QKV_LD + 768 + fk * 8;
        tkf[i][0] = *(const bf16x8*)kp;
        tkf[i][1] = *(const bf16x8*)(kp + 32);
      }
    }

    for (int qt = 0; qt < ntile; ++qt) {
      const int r = qt * 16 + frow;           // this lane's query row (MFMA column)
      const bool rvalid = r < R;
      const int lim = r < L ? r : r - L;      // the last token row it attends
      bf16x8 qf[2];
      {
        const bf16_t* qp = rows + (size_t)(rvalid ? r : 0) * QKV_LD + fk * 8;
        qf[0] = *(const bf16x8*)qp;
        qf[1] = *(const bf16x8*)(qp + 32);
        if (!rvalid) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { qf[0][j] = (__bf16)0.f; qf[1][j] = (__bf16)0.f; }
        }
      }
      // ---- scores: lane holds S[query frow][key kb*16 + fk*4 + e]
      float mx = -1e30f;
#pragma unroll
      for (int i = 0; i < GRID_MAXB; ++i) {
        const int kb = w + 4 * i;
        if (kb < GRID_NKB) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[i][0], qf[0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[i][1], qf[1], acc, 0, 0, 0);
          uint32_t mbits = 0xfu;              // this lane's four keys of the block, bit e = key e visible
          if (MASKED) {                       // the wave index through readfirstlane: the word's address is scalar, the load a scalar load
            const int kbu = __builtin_amdgcn_readfirstlane(w) + 4 * i;
            mbits = vis_mask[cap * GRID_MW + (kbu >> 1)] >> ((kbu & 1) * 16 + fk * 4);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = kb * 16 + fk * 4 + e;
            const float v = key < GRID_S && (!MASKED || ((mbits >> e) & 1u)) ? acc[e] : -INFINITY;
            sc[frow][key] = v;
            mx = fmaxf(mx, v);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kb = w + 4 * i;
        if (kb < ntile) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tkf[i][0], qf[0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tkf[i][1], qf[1], acc, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = kb * 16 + fk * 4 + e;
            // token keys up to the row's limit; a probe also sees itself; nobody else sees a probe
            const bool vis = rvalid && ((key < L && key <= lim) || (r >= L && key == r));
            const float v = vis ? acc[e] : -INFINITY;
            sc[frow][VT_KP + key] = v;
            mx = fmaxf(mx, v);
          }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      if (fk == 0) s_max[frow][w] = mx;
      __syncthreads();                        // scores, maxima (and, for the caption's first tile, s_vt)

      // ---- P . V.  Y = P (row = query frow, 8 keys at fk*8 of a 32-key block); lane holds O[query frow][dim db*16 + fk*4 + e]
      const float mrow = ceilf(fmaxf(fmaxf(s_max[frow][0], s_max[frow][1]), fmaxf(s_max[frow][2], s_max[frow][3])) * c_log2);
      f32x4 oacc[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
      float lsum = 0.f;
#pragma unroll
      for (int i = 0; i < GRID_MAXV; ++i) {
        const int kb = w + 4 * i;
        if (kb < GRID_NVB) {
          bf16x8 pf;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float p = fast_exp2(fmaf(sc[frow][kb * 32 + fk * 8 + e], c_log2, -mrow));
            lsum += p;
            pf[e] = (__bf16)p;
          }
#pragma unroll
          for (int db = 0; db < 4; ++db) oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[i][db], pf, oacc[db], 0, 0, 0);
        }
      }
      // text P.V block tb on wave 3 - tb (wave 3 owns one visual block fewer)
      if (w >= 1) {
        const int tb = 3 - w;
        if (tb * 32 < R) {
          bf16x8 pf;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float p = fast_exp2(fmaf(sc[frow][VT_KP + tb * 32 + fk * 8 + e], c_log2, -mrow));
            lsum += p;
            pf[e] = (__bf16)p;
          }
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            const bf16x8 tv = __builtin_bit_cast(bf16x8, *(const uint4*)&s_vt[db * 16 + frow][tb * 32 + fk * 8]);
            oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tv, pf, oacc[db], 0, 0, 0);
          }
        }
      }
      lsum += __shfl_xor(lsum, 16, 64);
      lsum += __shfl_xor(lsum, 32, 64);
      if (fk == 0) s_l[frow][w] = lsum;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 4; ++e) s_o[w * 16 + frow][db * 16 + fk * 4 + e] = oacc[db][e];
      __syncthreads();
      // ---- merge: out[q][d] = (sum over waves of the partial contexts) / (sum over waves of the row sums)
      for (int i = tid; i < 16 * HD; i += 256) {
        const int qn = i >> 6, d = i & 63, ro = qt * 16 + qn;
        if (ro < R) {
          const float l = (s_l[qn][0] + s_l[qn][1]) + (s_l[qn][2] + s_l[qn][3]);
          const float o = (s_o[qn][d] + s_o[16 + qn][d]) + (s_o[32 + qn][d] + s_o[48 + qn][d]);
          out[(cap * R + ro) * 768 + h * HD + d] = f2bf(o / l);
        }
      }
      // the next tile's writes need no further barrier: sc and s_max are rewritten only by waves that have passed the barrier above,
      // which every wave reaches after its last read of them; s_o / s_l are rewritten after the next tile's first barrier, which
      // every wave reaches after this merge
    }
  }
}

}  // namespace

extern "C" int vitcap_attn_text_grid(const void* qkv_text, const void* vis_qkv, const void* vis_vt, void* out, int n_images,
                                     int caps_per_image, int S_vis, int max_len, float scale, void* stream) {
  VC_REQUIRE(qkv_text && vis_qkv && vis_vt && out && n_images > 0, "attn_text_grid: bad arguments");
  VC_REQUIRE(((uintptr_t)qkv_text & 15) == 0 && ((uintptr_t)vis_qkv & 15) == 0 && ((uintptr_t)vis_vt & 15) == 0, "attn_text_grid: misaligned");
  VC_REQUIRE(S_vis == GRID_S, "attn_text_grid: S_vis must be %d (got %d)", GRID_S, S_vis);
  VC_REQUIRE(max_len >= 2 && max_len <= 40, "attn_text_grid: max_len must be 2..40 (got %d)", max_len);
  VC_REQUIRE(caps_per_image >= 1 && caps_per_image <= 32, "attn_text_grid: caps_per_image must be 1..32 (got %d)", caps_per_image);
  const int groups = (caps_per_image + GRID_G - 1) / GRID_G;
  VC_FUNC_SMEM(attn_text_grid_kernel<false>, (int)GRID_SMEM);
  hipLaunchKernelGGL(attn_text_grid_kernel<false>, dim3(NH, n_images * groups), dim3(256), GRID_SMEM, (hipStream_t)stream,
                     (const bf16_t*)qkv_text, (const bf16_t*)vis_qkv, (const bf16_t*)vis_vt, (bf16_t*)out, (const uint32_t*)nullptr,
                     caps_per_image, groups, max_len, scale * 1.4426950408889634f);
  VC_LAUNCH_CHECK("attn_text_grid");
  return VITCAP_OK;
}

extern "C" int vitcap_attn_text_grid_masked(const void* qkv_text, const void* vis_qkv, const void* vis_vt, const uint32_t* vis_mask,
                                            void* out, int n_images, int caps_per_image, int S_vis, int max_len, float scale,
                                            void* stream) {
  VC_REQUIRE(qkv_text && vis_qkv && vis_vt && out && n_images > 0, "attn_text_grid_masked: bad arguments");
  VC_REQUIRE(((uintptr_t)qkv_text & 15) == 0 && ((uintptr_t)vis_qkv & 15) == 0 && ((uintptr_t)vis_vt & 15) == 0,
             "attn_text_grid_masked: misaligned");
  VC_REQUIRE(vis_mask != nullptr, "attn_text_grid_masked: vis_mask is null");
  VC_REQUIRE(((uintptr_t)vis_mask & 3) == 0, "attn_text_grid_masked: vis_mask is not 4-byte aligned");
  VC_REQUIRE(S_vis == GRID_S, "attn_text_grid_masked: S_vis must be %d (got %d)", GRID_S, S_vis);
  VC_REQUIRE(max_len >= 2 && max_len <= 40, "attn_text_grid_masked: max_len must be 2..40 (got %d)", max_len);
  VC_REQUIRE(caps_per_image >= 1 && caps_per_image <= 32, "attn_text_grid_masked: caps_per_image must be 1..32 (got %d)", caps_per_image);
  const int groups = (caps_per_image + GRID_G - 1) / GRID_G;
  VC_FUNC_SMEM(attn_text_grid_kernel<true>, (int)GRID_SMEM);
  hipLaunchKernelGGL(attn_text_grid_kernel<true>, dim3(NH, n_images * groups), dim3(256), GRID_SMEM, (hipStream_t)stream,
                     (const bf16_t*)qkv_text, (const bf16_t*)vis_qkv, (const bf16_t*)vis_vt, (bf16_t*)out, vis_mask, caps_per_image, groups,
                     max_len, scale * 1.4426950408889634f);
  VC_LAUNCH_CHECK("attn_text_grid_masked");
  return VITCAP_OK;
}
