// Encoder attention rollout (include/vitcap_hip.h): the self-attention probabilities of a ViT block written out
// (vitcap_attn_self_maps -- the `attn` of timm's Attention.forward, vision_transformer.py:179-183, which vitcap_attn_dense_fwd forms
// and consumes inside its key loop), and one rollout step on a few row vectors (vitcap_rollout_step).  No P.V here: the dense kernel
// still computes the block's output.
//
// vitcap_attn_self_maps follows attn_probe_maps_kernel (attn_maps.hip); here the queries are the image's own rows and there are no
// token or self columns.  One workgroup (4 waves) per (16-query tile, image); it walks the 12 heads in the order 0..11:
//   * scores by mfma_f32_16x16x32_bf16, K fragment as A, the tile's 16 queries as B, two k-halves added in the accumulator: wave w
//     owns the 16-key blocks w, w + 4, ..; raw scores are staged in LDS;
//   * softmax in the log2 domain, m = ceil(max * c), p = exp2(s * c - m) kept in fp32; 16 lanes per row add the row sum (each lane its
//     columns in ascending order, then a 16-lane butterfly: the same order on every run) and write p / sum;
//   * per head: the row goes straight to `out`; head mean: the same lane adds head after head into an fp32 LDS row it alone owns and
//     writes sum * (1 / 12) after head 11 -- fixed order, no atomics, the same bits on every run.
// The LDS row lengths follow S (odd, so that rows start in different banks): at S = 577 / 578 the score stage is 16 x 593 fp32
// (37 952 B) and the head-mean form adds 16 x 579 (37 056 B) -- 75 KB, under half a CU's 160 KB; only S > 624 goes past that half.
// A tile whose rows all lie at or past q_rows writes its zeros and leaves.
#include <string.h>

#include "attn_common.h"

namespace {

constexpr int SM_SMAX = 640;                       // keys (and rows) per image at most
constexpr int RO_ROWS = 8;                         // rollout: rows of v per workgroup
constexpr int RO_RMAX = 64;

struct SelfMapArgs {
  const bf16_t* qkv;          // [B * S][2304]
  float* out;                 // [B][12 or 1][S][S]
  int S, q_rows, per_head;
  int sc_ld, acc_ld;          // floats per LDS row of the score stage / of the head-mean accumulator
  float c_log2;
};

__global__ __launch_bounds__(256) void attn_self_maps_kernel(SelfMapArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sm_smem[];
  float* sc = (float*)sm_smem;                                       // [16][sc_ld] raw scores, then p
  float* acc = sc + 16 * a.sc_ld;                                    // [16][acc_ld] sum over heads (head mean only: not allocated per head)
  __shared__ float s_max[16][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qt = blockIdx.x;
  const size_t img = blockIdx.y;
  const int frow = lane & 15, fk = lane >> 4;
  const int S = a.S, nkb = (S + 15) >> 4;
  const int nh_out = a.per_head ? NH : 1;
  // softmax ownership: 16 lanes per row
  const int srow = tid >> 4, sub = tid & 15;
  const int sq = qt * 16 + srow;                   // query row of the softmax group
  float* oimg = a.out + img * nh_out * (size_t)S * S;

  if (qt * 16 >= a.q_rows) {                       // nothing of this tile is asked for: zeros (uniform per workgroup)
    if (sq < S)
      for (int h = 0; h < nh_out; ++h) {
        float* orow = oimg + ((size_t)h * S + sq) * S;
        for (int col = sub; col < S; col += 16) orow[col] = 0.f;
      }
    return;
  }
  if (!a.per_head)
    for (int i = tid; i < 16 * a.acc_ld; i += 256) acc[i] = 0.f;

  const bf16_t* rows = a.qkv + img * S * QKV_LD;   // row r of this image: rows + r * QKV_LD (+ h * 64; +768 K)
  // this lane's query as MFMA column; a lane past the last asked row reads that row again (its column is never looked at)
  const int jq = qt * 16 + frow;
  const int qrow = jq < a.q_rows ? jq : a.q_rows - 1;
  const bool live = sq < a.q_rows;                 // uniform per 16-lane group

  for (int h = 0; h < NH; ++h) {
    // ---- scores: lane holds S[query frow][key kb*16 + fk*4 + e]
    bf16x8 qf[2];
    {
      const bf16_t* qp = rows + (size_t)qrow * QKV_LD + h * HD + fk * 8;
      qf[0] = *(const bf16x8*)qp;
      qf[1] = *(const bf16x8*)(qp + 32);
    }
    float mx = -1e30f;
    for (int kb = w; kb < nkb; kb += 4) {
      int key = kb * 16 + frow;
      key = key < S ? key : S - 1;
      const bf16_t* kp = rows + (size_t)key * QKV_LD + 768 + h * HD + fk * 8;
      const bf16x8 k0 = *(const bf16x8*)kp, k1 = *(const bf16x8*)(kp + 32);
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], s, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kb * 16 + fk * 4 + e;        // < nkb * 16 <= sc_ld
        const float v = k < S ? s[e] : -INFINITY;
        sc[frow * a.sc_ld + k] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (fk == 0) s_max[frow][w] = mx;
    __syncthreads();                               // scores and maxima (first head: acc, too)

    // ---- softmax of row srow by its 16 lanes
    if (sq < S) {
      float* orow = oimg + ((size_t)(a.per_head ? h : 0) * S + sq) * S;
      if (live) {
        const float mrow = ceilf(fmaxf(fmaxf(s_max[srow][0], s_max[srow][1]), fmaxf(s_max[srow][2], s_max[srow][3])) * a.c_log2);
        float* srw = sc + srow * a.sc_ld;
        float lsum = 0.f;
        for (int col = sub; col < S; col += 16) {
          const float p = fast_exp2(fmaf(srw[col], a.c_log2, -mrow));
          srw[col] = p;
          lsum += p;
        }
        lsum += __shfl_xor(lsum, 1, 64);
        lsum += __shfl_xor(lsum, 2, 64);
        lsum += __shfl_xor(lsum, 4, 64);
        lsum += __shfl_xor(lsum, 8, 64);
        if (a.per_head) {
          for (int col = sub; col < S; col += 16) orow[col] = srw[col] / lsum;
        } else {
          float* arow = acc + srow * a.acc_ld;
          for (int col = sub; col < S; col += 16) arow[col] += srw[col] / lsum;
        }
      } else if (a.per_head) {
        for (int col = sub; col < S; col += 16) orow[col] = 0.f;
      }
    }
    __syncthreads();                               // every lane has left sc / s_max before the next head's scores are staged
  }
  // head mean: heads were added in the order 0..11 by the lane that owns the column; rows past q_rows stayed 0
  if (!a.per_head && sq < S) {
    float* orow = oimg + (size_t)sq * S;
    const float* arow = acc + srow * a.acc_ld;
    for (int col = sub; col < S; col += 16) orow[col] = arow[col] * (1.0f / 12.0f);
  }
}

// One rollout step: v_out[b][r][k] = residual * v_in[b][r][k] + (1 - residual) * sum_j v_in[b][r][j] * A[b][j][k], j ascending.
// One workgroup (one wave) per (64 columns, 8 rows, image): the rows of v_in sit in LDS (every lane reads the same word: a
// broadcast), lane k walks column k of A from the top -- consecutive lanes read consecutive floats of one row of A -- and keeps the
// 8 sums in registers.  Plain fp32 multiply-adds in a fixed order: the same bits on every run.
__global__ __launch_bounds__(64) void rollout_step_kernel(const float* __restrict__ v_in, const float* __restrict__ A,
                                                          float* __restrict__ v_out, int rows, int S, float residual) {
  __shared__ float v[RO_ROWS][SM_SMAX];
  const int k = blockIdx.x * 64 + threadIdx.x;
  const int r0 = blockIdx.y * RO_ROWS;
  const size_t img = blockIdx.z;
  const int nr = rows - r0 < RO_ROWS ? rows - r0 : RO_ROWS;
  const float* vin = v_in + (img * rows + r0) * S;
  for (int i = threadIdx.x; i < RO_ROWS * S; i += 64) {
    const int r = i / S, j = i - r * S;
    v[r][j] = r < nr ? vin[(size_t)r * S + j] : 0.f;
  }
  __syncthreads();
  if (k >= S) return;
  const float* Ab = A + img * S * S + k;
  float acc[RO_ROWS];
#pragma unroll
  for (int r = 0; r < RO_ROWS; ++r) acc[r] = 0.f;
  for (int j = 0; j < S; ++j) {
    const float ajk = Ab[(size_t)j * S];
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) acc[r] = fmaf(v[r][j], ajk, acc[r]);
  }
  float* vo = v_out + (img * rows + r0) * S + k;
  const float mix = 1.0f - residual;
#pragma unroll
  for (int r = 0; r < RO_ROWS; ++r)
    if (r < nr) vo[(size_t)r * S] = fmaf(residual, v[r][k], mix * acc[r]);
}

}  // namespace

extern "C" int vitcap_attn_self_maps(const void* qkv, float* out, int B, int S, int q_rows, float scale, int per_head, void* stream) {
  VC_REQUIRE(qkv && out, "attn_self_maps: null %s", qkv ? "out" : "qkv");
  VC_REQUIRE(((uintptr_t)qkv & 15) == 0, "attn_self_maps: qkv not 16-byte aligned");
  VC_REQUIRE(((uintptr_t)out & 3) == 0, "attn_self_maps: out not 4-byte aligned");
  VC_REQUIRE(B > 0 && B <= 65535, "attn_self_maps: B must be 1..65535 (got %d)", B);
  VC_REQUIRE(S >= 1 && S <= SM_SMAX, "attn_self_maps: S must be 1..%d (got %d)", SM_SMAX, S);
  VC_REQUIRE(q_rows >= 1 && q_rows <= S, "attn_self_maps: q_rows must be 1..S = %d (got %d)", S, q_rows);
  VC_REQUIRE(per_head == 0 || per_head == 1, "attn_self_maps: per_head must be 0 or 1 (got %d)", per_head);
  const int nkb = (S + 15) / 16;
  SelfMapArgs a{(const bf16_t*)qkv, out, S, q_rows, per_head, nkb * 16 + 1, S | 1, scale * 1.4426950408889634f};
  const size_t smem_sc = (size_t)16 * a.sc_ld * 4, smem_all = smem_sc + (size_t)16 * a.acc_ld * 4;
  VC_FUNC_SMEM(attn_self_maps_kernel, 16 * (SM_SMAX + 1) * 4 * 2);
  hipLaunchKernelGGL(attn_self_maps_kernel, dim3(nkb, (unsigned)B), dim3(256), per_head ? smem_sc : smem_all, (hipStream_t)stream, a);
  VC_LAUNCH_CHECK("attn_self_maps");
  return VITCAP_OK;
}

extern "C" int vitcap_rollout_step(const float* v_in, const float* A, float* v_out, int n_img, int rows, int S, float residual,
                                   void* stream) {
  VC_REQUIRE(v_in && A && v_out, "rollout_step: null %s", !v_in ? "v_in" : (!A ? "A" : "v_out"));
  VC_REQUIRE(((uintptr_t)v_in & 3) == 0 && ((uintptr_t)A & 3) == 0 && ((uintptr_t)v_out & 3) == 0,
             "rollout_step: v_in / A / v_out not 4-byte aligned");
  VC_REQUIRE(n_img > 0 && n_img <= 65535, "rollout_step: n_img must be 1..65535 (got %d)", n_img);
  VC_REQUIRE(rows >= 1 && rows <= RO_RMAX, "rollout_step: rows must be 1..%d (got %d)", RO_RMAX, rows);
  VC_REQUIRE(S >= 1 && S <= SM_SMAX, "rollout_step: S must be 1..%d (got %d)", SM_SMAX, S);
  {
    // on the bits: this file is built with -fno-honor-nans, under which a comparison may be assumed never to see a NaN
    uint32_t rb;
    memcpy(&rb, &residual, 4);
    VC_REQUIRE(rb <= 0x3f800000u || rb == 0x80000000u, "rollout_step: residual must be in [0, 1] (got %g)", (double)residual);
  }
  {
    const size_t n = (size_t)n_img * rows * S * 4;
    const uintptr_t i0 = (uintptr_t)v_in, o0 = (uintptr_t)v_out;
    VC_REQUIRE(i0 + n <= o0 || o0 + n <= i0, "rollout_step: v_out overlaps v_in");
  }
  hipLaunchKernelGGL(rollout_step_kernel, dim3((S + 63) / 64, (rows + RO_ROWS - 1) / RO_ROWS, (unsigned)n_img), dim3(64), 0,
                     (hipStream_t)stream, v_in, A, v_out, rows, S, residual);
  VC_LAUNCH_CHECK("rollout_step");
  return VITCAP_OK;
}
