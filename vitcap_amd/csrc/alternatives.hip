// Token alternatives of given captions (vitcap_score_rows_alts, include/vitcap_hip.h): per probe row of the one-pass scorer the k
// best vocabulary entries with their log-probs, the rank of the scored token and the entropy of the row.
#include "common.h"
#include "select.h"
#include "score_row.h"

namespace {

constexpr int ALT_PT = 32;              // row elements per thread: V <= 32 * 1024
constexpr int ALT_CAP = ALT_PT * 16;    // at most k <= 16 threads own an element of the list

struct AltArgs {
  int32_t* ids;      // [n_caps][L][k]
  float* lp;         // [n_caps][L][k]
  int32_t* rank;     // [n_caps][L]
  float* entropy;    // [n_caps][L]
  int k;
};

// -0.0 -> +0.0: the order of the alternatives is float comparison (-0 == +0, lower index first), tk_key alone puts +0 above -0
__device__ __forceinline__ float alt_canon(float x) { return x == 0.f ? 0.f : x; }

// the number of lanes of the wave that hold a larger key: 64 lane broadcasts, no dependent chain (wave_take_k costs a butterfly per
// extracted element)
__device__ __forceinline__ int wave_rank_u64(unsigned long long key) {
  int r = 0;
#pragma unroll
  for (int l = 0; l < 64; ++l) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)key, l), hi = __builtin_amdgcn_readlane((unsigned)(key >> 32), l);
    r += ((((unsigned long long)hi << 32) | lo) > key) ? 1 : 0;
  }
  return r;
}

// One 1024-thread workgroup per probe row.  The row is read ONCE, element tid + j * 1024 into register x[j]; the maximum, S, T, the
// rank count and the k best all come from those registers:
//   1. every thread's best element (Pick: larger value, lower index on ties), the workgroup's -> m and the argmax;
//   2. S = sum exp(x - m), T = sum exp(x - m) (x - m): score_rows_kernel's partial sums and block_sum<16>, so S has its bits;
//      S - 1 (the sum without the maximum's term) next to it, for the entropy's log S;
//   3. threshold selection as row_topk_lse_kernel: the k-th largest of the 1024 thread bests is a bound below which no element of
//      the row's top k lies, and exactly k threads own an element at or above it: those elements (<= 32 k) go to a list in LDS,
//      compared as floats -- a 64-bit key is built once per thread for the thread best and once per listed element;
//   4. in the same sweep every thread counts its elements that come before the scored token f.
// Keys are unique, so "the r-th best" is "the key with r larger ones": every selection here is a count taken by all candidates at
// once -- in a wave by lane broadcasts, across waves over a short LDS list -- instead of k rounds of extraction in one wave, whose
// cost (a 64-bit butterfly per round, three times, fifteen waves waiting) grew with k.
// SCORE: the kernel also writes what score_rows_kernel writes for the row (the engine's fused form: the chunk is read once).
template <bool SCORE>
__global__ __launch_bounds__(1024) void score_rows_alts_kernel(const float* __restrict__ logits, int ldl, int V, ScoreArgs a, AltArgs q,
                                                               int rows0) {
  __shared__ unsigned long long s_cand[16][16];      // [wave][round], k <= 16
  __shared__ unsigned long long s_list[ALT_CAP];
  __shared__ unsigned long long s_thr;
  __shared__ float s_v[16], s_sum[16], s_xf;
  __shared__ int s_i[16], s_cnt[16], s_n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, k = q.k;
  if (tid < 256) (&s_cand[0][0])[tid] = 0ull;         // a wave with fewer than k elements leaves slots empty (barriers follow)
  int b, t;
  score_row_place(rows0 + blockIdx.x, a.L, b, t);
  const int64_t* cap = a.ids + (size_t)b * a.L;
  const size_t o = (size_t)b * a.L + t;
  if (score_row_ended(cap, t, a.eos, a.eos_x)) {      // behind the end: the dead pattern
    if (tid < k) {
      q.ids[o * k + tid] = -1;
      q.lp[o * k + tid] = 0.f;
    }
    if (tid == 0) {
      q.rank[o] = -1;
      q.entropy[o] = 0.f;
      if constexpr (SCORE) score_row_write_dead(a, b, t);
    }
    return;
  }
  const float* row = logits + (size_t)blockIdx.x * ldl;
  float x[ALT_PT];
#pragma unroll
  for (int j = 0; j < ALT_PT; ++j) {
    const int i = tid + j * 1024;
    x[j] = i < V ? row[i] : -INFINITY;      // past the row's end: below every (finite) logit, exp(x - m) = 0, never listed or counted
  }
  Pick<false, false> mine;
#pragma unroll
  for (int j = 0; j < ALT_PT; ++j) mine.offer(x[j], tid + j * 1024);
  const Pick<false, false> best = block_pick<16>(mine, {s_v, s_i, nullptr, nullptr});
  const float m = best.v;
  float se = 0.f, sd = 0.f, te = 0.f;
#pragma unroll
  for (int j = 0; j < ALT_PT; ++j) {
    const float e = score_row_term(x[j], m);
    se += e;                                  // + 0 past the row's end: S keeps score_rows_kernel's bits
    sd += tid + j * 1024 == best.i ? 0.f : e; // S - 1: the same sum without the maximum's own term, which is exactly 1
    te += e > 0.f ? e * (x[j] - m) : 0.f;     // 0 * -inf past the row's end; an underflowed term is 0 either way
  }
  const float S = block_sum<16>(se, s_sum);
  const float S1 = block_sum<16>(sd, s_sum);
  const float T = block_sum<16>(te, s_sum);
  const int f = score_row_token(cap, a.last_tok, b, t, a.L, a.eos, V, best.i);
  if (tid == (f & 1023)) {                            // the owner of x[f] hands it to everyone
    float v = x[0];
#pragma unroll
    for (int j = 1; j < ALT_PT; ++j) v = j == (f >> 10) ? x[j] : v;
    s_xf = v;
  }
  if (tid == 0) s_n = 0;
  {                                                   // the k best thread bests of this wave, in order
    const unsigned long long mk = tid < V ? tk_key(alt_canon(mine.v), mine.i) : 0ull;
    const int r = wave_rank_u64(mk);
    if (mk != 0ull && r < k) s_cand[w][r] = mk;
  }
  __syncthreads();
  if (tid < 256 && (tid & 15) < k) {                  // the k-th largest of the 16 k candidates: the one with k - 1 larger ones
    const unsigned long long c = s_cand[tid >> 4][tid & 15];
    int r = 0;
    for (int u = 0; u < 16; ++u)
      for (int v = 0; v < k; ++v) r += s_cand[u][v] > c ? 1 : 0;
    if (c != 0ull && r == k - 1) s_thr = c;           // the launcher requires V >= k, so k thread bests exist
  }
  __syncthreads();
  const float xf = s_xf, tv = tk_val(s_thr);
  const int ti = tk_idx(s_thr);
  int before = 0;
#pragma unroll
  for (int j = 0; j < ALT_PT; ++j) {
    const int i = tid + j * 1024;
    before += (x[j] > xf || (x[j] == xf && i < f)) ? 1 : 0;
    if (x[j] > tv || (x[j] == tv && i <= ti)) {
      const int pos = atomicAdd(&s_n, 1);
      if (pos < ALT_CAP) s_list[pos] = tk_key(alt_canon(x[j]), i);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
  if (lane == 0) s_cnt[w] = before;
  __syncthreads();                                    // publishes the list and the counts
  const int n = s_n < ALT_CAP ? s_n : ALT_CAP;        // k <= n: the k thread bests at or above the threshold are on the list
  // tk_val gives the canonicalised value: for x = -0 the first term is (+0 - m) instead of (-0 - m).  The two differ only when m is
  // a zero too, and then only in the sign of a zero from which log S is subtracted: log S > 0 whenever a second zero is in the row,
  // and a lone -0 maximum gives +0 either way.  So the log-prob of the scored token has score_row_lp(x[f], m, S)'s bits.
  if (tid < n) {                                      // the list's entry with r larger ones is the r-th alternative
    const unsigned long long key = s_list[tid];
    int r = 0;
    for (int u = 0; u < n; ++u) r += s_list[u] > key ? 1 : 0;
    if (r < k) {
      q.ids[o * k + r] = tk_idx(key);
      q.lp[o * k + r] = score_row_lp(tk_val(key), m, S);
    }
  }
  if (tid == 0) {
    int rk = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) rk += s_cnt[u];
    q.rank[o] = rk;
    // log S as log1p(S - 1): on a confident row S - 1 << 1 is lost in S itself (1 + 2e-8 is 1 in fp32), and with it every digit of
    // log S; S - 1 summed on its own keeps the entropy's relative accuracy there
    q.entropy[o] = log1pf(S1) - T / S;
    if constexpr (SCORE) score_row_write(a, b, t, f, score_row_lp(xf, m, S));
  }
}

}  // namespace

int vc_score_rows_alts(const float* logits, int ldl, int V, const int64_t* caption_ids, const int64_t* last_tok, int rows0, int n_rows,
                       int n_caps, int max_len, int eos, const int32_t* eos_extra, int pad, float* token_logprobs, int64_t* out_ids,
                       int64_t* out_last_tok, float* logprob_out, int k, int32_t* alt_ids, float* alt_lp, int32_t* rank, float* entropy,
                       void* stream) {
  const bool score = token_logprobs != nullptr;
  VC_REQUIRE(logits && caption_ids && alt_ids && alt_lp && rank && entropy, "score_rows_alts: null pointer");
  VC_REQUIRE(!score || (out_ids && logprob_out), "score_rows_alts: null score outputs");
  VC_REQUIRE(k >= 1 && k <= 16, "score_rows_alts: k must be 1..16 (got %d)", k);
  VC_REQUIRE(V >= k && V <= ALT_PT * 1024 && ldl >= V && n_caps > 0 && max_len >= 2 && max_len <= 40,
             "score_rows_alts: bad sizes (V=%d, ldl=%d, max_len=%d)", V, ldl, max_len);
  VC_REQUIRE(rows0 >= 0 && n_rows > 0 && (long long)rows0 + n_rows <= (long long)n_caps * (max_len - 1),
             "score_rows_alts: rows [%d, %d + %d) outside the %d x %d probe rows", rows0, rows0, n_rows, n_caps, max_len - 1);
  ScoreArgs a{caption_ids, last_tok, token_logprobs, out_ids, out_last_tok, nullptr, nullptr, logprob_out, max_len, eos, pad,
              VcEosExtra{{eos_extra ? eos_extra[0] : -1, eos_extra ? eos_extra[1] : -1, eos_extra ? eos_extra[2] : -1}}};
  AltArgs q{alt_ids, alt_lp, rank, entropy, k};
  if (score)
    hipLaunchKernelGGL(score_rows_alts_kernel<true>, dim3(n_rows), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V, a, q, rows0);
  else
    hipLaunchKernelGGL(score_rows_alts_kernel<false>, dim3(n_rows), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V, a, q, rows0);
  VC_LAUNCH_CHECK("score_rows_alts");
  return score ? vc_score_finish(a, n_caps, rows0, n_rows, stream) : VITCAP_OK;
}

extern "C" int vitcap_score_rows_alts(const float* logits, int ldl, int V, const int64_t* caption_ids, const int64_t* last_tok, int rows0,
                                      int n_rows, int n_caps, int max_len, int eos, const int32_t* eos_extra, int pad, int k,
                                      int32_t* alt_ids, float* alt_lp, int32_t* rank, float* entropy, void* stream) {
  return vc_score_rows_alts(logits, ldl, V, caption_ids, last_tok, rows0, n_rows, n_caps, max_len, eos, eos_extra, pad, nullptr, nullptr,
                            nullptr, nullptr, k, alt_ids, alt_lp, rank, entropy, stream);
}
