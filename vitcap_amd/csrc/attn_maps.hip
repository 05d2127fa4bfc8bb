// Attention maps of the [MASK] probes of given captions (vitcap_attn_probe_maps, include/vitcap_hip.h): the normalised softmax rows
// that vitcap_attn_text_grid (attn_grid.hip) forms and consumes inside its query tiles, written out.  No P.V here -- the grid kernel
// still computes the layer's output.
//
// Only the probe rows are queries: probe j = 0..L-2 (grid row L + j, position t = j + 1) attends the image's 578 visual rows, token
// rows 0..j and itself (modeling_bert.py:846-876 at step cur_len = t).  The row that is written has width W = 578 + L:
//   columns 0..577 the visual keys in the cache's order, 578 + k (k < t) token key k, 578 + t the probe's own key, the rest exactly 0.
//
// One workgroup (4 waves) per (16-probe query tile, caption); it walks the 12 heads in the order 0..11:
//   * scores exactly as the grid kernel forms them (mfma_f32_16x16x32_bf16, K fragment as A, the 16 probes as B, two k-halves added in
//     the accumulator): wave w owns the visual 16-key blocks w, w + 4, ..; waves 0..2 the token blocks 0..2, wave 3 the block of the
//     tile's own 16 probe keys, whose diagonal holds the self scores; raw scores are staged in LDS;
//   * softmax in the log2 domain, m = ceil(max * c), p = exp2(s * c - m) kept in fp32; 16 lanes per row add the row sum (each lane its
//     columns in ascending order, then a 16-lane butterfly: the same order on every run) and write p / sum;
//   * per head: the row goes straight to `out`; head mean: the same lane adds head after head into an fp32 LDS row it alone owns and
//     writes sum * (1 / 12) after head 11 -- fixed order, no atomics, the same bits on every run.  That accumulator is half of the
//     head-mean form's 81 KB of LDS; the per-head form asks for the 41 KB of the score stage only.
// Position 0 and every position behind the caption's first end token hold no decision: their rows are written as zeros.
#include "attn_common.h"

namespace {

constexpr int MAP_S = 578;                         // visual rows per image
constexpr int MAP_NKB = (MAP_S + 15) / 16;         // 37 visual score blocks
constexpr int MAP_MAXB = (MAP_NKB + 3) / 4;        // 10 per wave
constexpr int MAP_TOK0 = MAP_NKB * 16;             // 592: first token score column (3 blocks of 16 token keys, L <= 40)
constexpr int MAP_SELF = MAP_TOK0 + 48;            // 640: the probe's own score
constexpr int MAP_SC_LD = MAP_SELF + 5;            // 645 fp32 per query row (odd: rows start in different LDS banks)
constexpr int MAP_LMAX = 40;
constexpr int MAP_ACC_LD = MAP_S + MAP_LMAX + 1;   // 619 fp32 per row of the head-mean accumulator (odd)
constexpr size_t MAP_SMEM_SC = (size_t)16 * MAP_SC_LD * 4;                                  // 41 280 B: all the per-head form needs
constexpr size_t MAP_SMEM = MAP_SMEM_SC + (size_t)16 * MAP_ACC_LD * 4;                      // 80 896 B with the head-mean accumulator

struct MapArgs {
  const bf16_t* qkv_text;     // [n_caps][2L-1][2304]
  const bf16_t* vis_qkv;      // [n_images * 578][2304]
  const int64_t* ids;         // [n_caps][L]
  float* out;                 // one layer's slice of [n_caps][L][4]([12])[W]
  int caps_per_image, L, per_head, eos;
  VcEosExtra eos_x;
  float c_log2;
};

__global__ __launch_bounds__(256) void attn_probe_maps_kernel(MapArgs a) {
  extern __shared__ __attribute__((aligned(16))) char map_smem[];
  float (*sc)[MAP_SC_LD] = (float (*)[MAP_SC_LD])map_smem;                                          // [16][645] raw scores, then p
  float (*acc)[MAP_ACC_LD] = (float (*)[MAP_ACC_LD])(map_smem + MAP_SMEM_SC);      // [16][619] sum over heads (head mean only: not allocated per head)
  __shared__ float s_max[16][4];
  __shared__ int s_live[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qt = blockIdx.x;
  const size_t cap = blockIdx.y;
  const int img = (int)(cap / a.caps_per_image);
  const int frow = lane & 15, fk = lane >> 4;
  const int L = a.L, R = 2 * L - 1, W = MAP_S + L;
  const int ntok = (L + 15) >> 4;                  // token score blocks (<= 3)
  const size_t row_ld = (size_t)4 * (a.per_head ? NH : 1) * W;      // floats between positions t and t + 1 of the full array
  const int64_t* capids = a.ids + cap * L;
  float* ocap = a.out + cap * L * row_ld;

  // which of the tile's probes hold a decision: position t = qt * 16 + q + 1 inside the caption, no end token strictly before it
  if (tid < 16) {
    const int t = qt * 16 + tid + 1;
    bool live = t < L;
    for (int j = 1; j < t && j < L; ++j) live = live && !vc_is_eos((int)capids[j], a.eos, a.eos_x);
    s_live[tid] = live ? 1 : 0;
  }
  if (!a.per_head)
    for (int i = tid; i < 16 * MAP_ACC_LD; i += 256) (&acc[0][0])[i] = 0.f;
  // position 0 holds no decision: zeros (written by the caption's first tile)
  if (qt == 0) {
    const int n = (a.per_head ? NH : 1) * W;
    for (int i = tid; i < n; i += 256) ocap[i] = 0.f;
  }

  const bf16_t* rows = a.qkv_text + cap * R * QKV_LD;      // row r of this caption: rows + r * QKV_LD (+ h * 64; +768 K)
  // this lane's probe as MFMA column: probe j = qt * 16 + frow, grid row L + j
  const int jq = qt * 16 + frow;
  const bool qvalid = jq < L - 1;
  const int qrow = L + (qvalid ? jq : L - 2);
  // softmax ownership: 16 lanes per row
  const int srow = tid >> 4, sub = tid & 15;
  const int st = qt * 16 + srow + 1;               // position of row srow
  const int ncol = MAP_S + st + 1;                 // live columns of that row (<= W when st < L)

  for (int h = 0; h < NH; ++h) {
    // ---- scores: lane holds S[query frow][key kb*16 + fk*4 + e]
    bf16x8 qf[2];
    {
      const bf16_t* qp = rows + (size_t)qrow * QKV_LD + h * HD + fk * 8;
      qf[0] = *(const bf16x8*)qp;
      qf[1] = *(const bf16x8*)(qp + 32);
    }
    float mx = -1e30f;
#pragma unroll
    for (int i = 0; i < MAP_MAXB; ++i) {
      const int kb = w + 4 * i;
      if (kb < MAP_NKB) {
        int key = kb * 16 + frow;
        key = key < MAP_S ? key : MAP_S - 1;
        const bf16_t* kp = a.vis_qkv + ((size_t)img * MAP_S + key) * QKV_LD + 768 + h * HD + fk * 8;
        const bf16x8 k0 = *(const bf16x8*)kp, k1 = *(const bf16x8*)(kp + 32);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kb * 16 + fk * 4 + e;
          const float v = k < MAP_S ? s[e] : -INFINITY;
          sc[frow][k] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    {
      // waves 0..2: token block w (keys w*16 ..); wave 3: the tile's own probe keys (grid rows L + qt*16 ..), diagonal only
      const bool tokblk = w < 3;
      if (!tokblk || w < ntok) {
        int key = tokblk ? w * 16 + frow : L + qt * 16 + frow;
        const int kmax = tokblk ? L - 1 : R - 1;
        key = key < kmax ? key : kmax;
        const bf16_t* kp = rows + (size_t)key * QKV_LD + 768 + h * HD + fk * 8;
        const bf16x8 k0 = *(const bf16x8*)kp, k1 = *(const bf16x8*)(kp + 32);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = fk * 4 + e;               // key within the block
          if (tokblk) {
            const int k = w * 16 + kk;
            const bool vis = qvalid && k <= jq;    // token keys 0..j = 0..t-1
            const float v = vis ? s[e] : -INFINITY;
            sc[frow][MAP_TOK0 + k] = v;
            mx = fmaxf(mx, v);
          } else if (kk == frow) {
            sc[frow][MAP_SELF] = s[e];
            mx = fmaxf(mx, s[e]);
          }
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (fk == 0) s_max[frow][w] = mx;
    __syncthreads();                               // scores and maxima (first head: s_live, acc, too)

    // ---- softmax of row srow by its 16 lanes
    if (st < L) {                                  // uniform per 16-lane group
      float* orow = ocap + (size_t)st * row_ld + (a.per_head ? (size_t)h * W : 0);
      if (s_live[srow]) {
        const float mrow = ceilf(fmaxf(fmaxf(s_max[srow][0], s_max[srow][1]), fmaxf(s_max[srow][2], s_max[srow][3])) * a.c_log2);
        float lsum = 0.f;
        for (int col = sub; col < ncol; col += 16) {
          const int k = col < MAP_S ? col : (col < ncol - 1 ? MAP_TOK0 + (col - MAP_S) : MAP_SELF);
          const float p = fast_exp2(fmaf(sc[srow][k], a.c_log2, -mrow));
          sc[srow][k] = p;
          lsum += p;
        }
        lsum += __shfl_xor(lsum, 1, 64);
        lsum += __shfl_xor(lsum, 2, 64);
        lsum += __shfl_xor(lsum, 4, 64);
        lsum += __shfl_xor(lsum, 8, 64);
        if (a.per_head) {
          for (int col = sub; col < W; col += 16) {
            const int k = col < MAP_S ? col : (col < ncol - 1 ? MAP_TOK0 + (col - MAP_S) : MAP_SELF);
            orow[col] = col < ncol ? sc[srow][k] / lsum : 0.f;
          }
        } else {
          for (int col = sub; col < ncol; col += 16) {
            const int k = col < MAP_S ? col : (col < ncol - 1 ? MAP_TOK0 + (col - MAP_S) : MAP_SELF);
            acc[srow][col] += sc[srow][k] / lsum;
          }
        }
      } else if (a.per_head) {
        for (int col = sub; col < W; col += 16) orow[col] = 0.f;
      }
    }
    __syncthreads();                               // every lane has left sc / s_max before the next head's scores are staged
  }
  // head mean: heads were added in the order 0..11 by the lane that owns the column; dead rows and dead columns stayed 0
  if (!a.per_head && st < L) {
    float* orow = ocap + (size_t)st * row_ld;
    for (int col = sub; col < W; col += 16) orow[col] = acc[srow][col] * (1.0f / 12.0f);
  }
}

}  // namespace

extern "C" int vitcap_attn_probe_maps(const void* qkv_text, const void* vis_qkv, const int64_t* caption_ids, float* out, int n_images,
                                      int caps_per_image, int S_vis, int max_len, int per_head, int eos, const int32_t* eos_extra,
                                      float scale, void* stream) {
  VC_REQUIRE(qkv_text && vis_qkv && caption_ids && out && n_images > 0,
             "attn_probe_maps: null qkv_text / vis_qkv / caption_ids / out, or n_images <= 0");
  VC_REQUIRE(((uintptr_t)qkv_text & 15) == 0 && ((uintptr_t)vis_qkv & 15) == 0, "attn_probe_maps: qkv_text / vis_qkv not 16-byte aligned");
  VC_REQUIRE(((uintptr_t)caption_ids & 7) == 0 && ((uintptr_t)out & 3) == 0, "attn_probe_maps: caption_ids / out misaligned");
  VC_REQUIRE(S_vis == MAP_S, "attn_probe_maps: S_vis must be %d (got %d)", MAP_S, S_vis);
  VC_REQUIRE(max_len >= 2 && max_len <= MAP_LMAX, "attn_probe_maps: max_len must be 2..40 (got %d)", max_len);
  VC_REQUIRE(caps_per_image >= 1 && caps_per_image <= 32, "attn_probe_maps: caps_per_image must be 1..32 (got %d)", caps_per_image);
  VC_REQUIRE(per_head == 0 || per_head == 1, "attn_probe_maps: per_head must be 0 or 1 (got %d)", per_head);
  const long long n_caps = (long long)n_images * caps_per_image;
  VC_REQUIRE(n_caps <= 65535, "attn_probe_maps: n_images * caps_per_image must be <= 65535 (got %lld)", n_caps);
  MapArgs a{(const bf16_t*)qkv_text, (const bf16_t*)vis_qkv, caption_ids, out, caps_per_image, max_len, per_head, eos,
            VcEosExtra{{eos_extra ? eos_extra[0] : -1, eos_extra ? eos_extra[1] : -1, eos_extra ? eos_extra[2] : -1}},
            scale * 1.4426950408889634f};
  VC_FUNC_SMEM(attn_probe_maps_kernel, (int)MAP_SMEM);
  hipLaunchKernelGGL(attn_probe_maps_kernel, dim3((max_len - 1 + 15) / 16, (unsigned)n_caps), dim3(256), per_head ? MAP_SMEM_SC : MAP_SMEM,
                     (hipStream_t)stream, a);
  VC_LAUNCH_CHECK("attn_probe_maps");
  return VITCAP_OK;
}
