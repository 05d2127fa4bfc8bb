// Greedy bookkeeping and tag top-k: row-wise scans over the 30522-wide vocabulary (HBM/L2-bound).
#include "common.h"
#include "rng.h"
#include "select.h"
#include "score_row.h"

namespace {

__global__ void greedy_init_kernel(int64_t* ids, int32_t* unf, float* sum_lp, float* cnt, int B, int max_len, int bos,
                                   int pad, int32_t* live) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && live) *live = B;            // sequences still unfinished (decode kernels return at entry once it is 0)
  if (i < B * max_len) ids[i] = (i % max_len == 0) ? bos : pad;
  if (i < B) {
    unf[i] = 1;
    sum_lp[i] = 0.f;
    cnt[i] = 0.f;
  }
}

// one 1024-thread workgroup per sequence
__global__ __launch_bounds__(1024) void greedy_step_kernel(const float* __restrict__ logits, int ldl, int V, StepState st, int t) {
  __shared__ float s_v[16], s_second[16], s_sum[16];
  __shared__ int s_i[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  // a finished sequence's logits are not read -- once every sequence has finished the step's other kernels have not even produced them
  if (st.skip_finished(b, t)) return;
  const float* row = logits + (size_t)b * ldl;
  Pick<true, false> best;                  // with the runner-up, for the top-2 margin tap
  for (int i = tid; i < V; i += 1024) best.offer(row[i], i);
  best = block_pick<16>(best, {s_v, s_i, s_second, nullptr});
  float se = 0.f;
  for (int i = tid; i < V; i += 1024) se += expf(row[i] - best.v);
  const float tot = block_sum<16>(se, s_sum);
  if (tid != 0) return;
  const int f = st.forced_at(b, t, V);
  // log-prob = logit[tok] - max - log(sum exp(x - max)); the free choice is the max itself.  A forced token is scored on the same
  // row with the same max and sum, so forcing the argmax gives the free choice's own value.
  if (f < 0) st.commit(b, t, best.i, -logf(tot), best.v - best.second);
  else st.commit(b, t, f, (row[f] - best.v) - logf(tot), best.v - best.second, st.score_forced != 0);
}


// ---- sampling step (do_sample): temperature, top-k / top-p filtering, one draw per sequence ----------------------
// One 1024-thread workgroup per sequence; the whole 30522-wide row lives in registers (30 values per thread).
constexpr int SM_NPT = 30;
struct SampleArgs {
  const float* logits;
  int ldl, V;
  float temperature;
  int top_k;
  float top_p;
  uint32_t seed;
  int seq_off;      // row b draws from the stream of sequence b + seq_off of the call
};
struct SampleLds {
  RadixLds radix;
  float f[16];
};

// The front end both sampling kernels share: row b scaled by 1 / temperature into x (element j = column tid + 1024 j; key = its
// order key, 0 beyond V), top-k with k = max(top_k, min_keep), top-p keeping ranks 0..min_keep whatever their mass
// (min_tokens_to_keep, modeling_utils.py:1125-1130).  Survivors are the elements with key >= the returned threshold;
// m = their maximum, z = sum exp(x - m) over them.
__device__ __forceinline__ uint32_t sample_filter(const SampleArgs& a, int b, int min_keep, float (&x)[SM_NPT],
                                                   uint32_t (&key)[SM_NPT], float& m, float& z, SampleLds& lds) {
  const int tid = threadIdx.x;
  const float* row = a.logits + (size_t)b * a.ldl;
#pragma unroll
  for (int j = 0; j < SM_NPT; ++j) {
    const int i = tid + j * 1024;
    float v = i < a.V ? row[i] : -INFINITY;
    if (a.temperature != 1.0f) v = v / a.temperature;
    x[j] = v;
    key[j] = i < a.V ? order_key(v) : 0u;
  }
  uint32_t thr = 1u;                                       // keep every present element
  if (a.top_k > 0) {
    const int top_k = a.top_k < min_keep ? min_keep : a.top_k;
    const uint32_t tk = radix_select(key, [](int) { return 1ull; }, (unsigned long long)(top_k < a.V ? top_k : a.V) - 1ull, lds.radix);
    thr = tk > thr ? tk : thr;
  }
  // softmax statistics of the surviving set
  auto mass = [&](uint32_t from) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < SM_NPT; ++j) if (key[j] >= from) s += expf(x[j] - m);
    return block_sum<16>(s, lds.f);
  };
  m = -INFINITY;
#pragma unroll
  for (int j = 0; j < SM_NPT; ++j) if (key[j] >= thr) m = fmaxf(m, x[j]);
  m = block_max<16>(m, lds.f);
  z = mass(thr);
  if (a.top_p < 1.0f) {                                    // nucleus
    const float scale = 1099511627776.0f / z;              // 2^40 / Z: probabilities as 40-bit fixed point
    const unsigned long long P = (unsigned long long)((double)a.top_p * 1099511627776.0);
    const uint32_t thr_k = thr;
    uint32_t tp = radix_select(key, [&](int j) { return key[j] >= thr_k ? (unsigned long long)(expf(x[j] - m) * scale) : 0ull; }, P,
                               lds.radix);
    if (min_keep > 1) {                                    // ranks 0..min_keep stay whatever their mass
      const uint32_t tm = radix_select(key, [&](int j) { return key[j] >= thr_k ? 1ull : 0ull; }, (unsigned long long)min_keep,
                                       lds.radix);
      tp = tm < tp ? tm : tp;
    }
    if (tp > thr) {
      thr = tp;
      z = mass(thr);                                       // renormalise over the nucleus
    }
  }
  return thr;
}
// noise stream of row b at step t, and the score of its column i: x + Gumbel noise, so that argmax == multinomial(softmax(x))
__device__ __forceinline__ uint32_t sample_stream(const SampleArgs& a, int b, int t) {
  return vc_mix(vc_mix(a.seed, (uint32_t)(b + a.seq_off)), (uint32_t)t);
}
__device__ __forceinline__ float gumbel_score(float x, uint32_t hrow, int i) {
  return x - logf(-logf(vc_uniform(vc_mix(hrow, (uint32_t)i))));
}

// A forced token under sampling: nothing is filtered and nothing is drawn.  Its log-prob is log_softmax(logits / temperature)[f]
// over the WHOLE row -- the top-k / top-p filter would score a token it removes at -inf.  Every thread of the workgroup calls it.
__device__ __forceinline__ void sample_take_forced(const SampleArgs& a, const StepState& st, int b, int t, int f, float* lds_f) {
  const int tid = threadIdx.x;
  const float* row = a.logits + (size_t)b * a.ldl;
  auto scaled = [&](int i) { const float v = row[i]; return a.temperature != 1.0f ? v / a.temperature : v; };
  float m = -INFINITY;
  for (int i = tid; i < a.V; i += 1024) m = fmaxf(m, scaled(i));
  m = block_max<16>(m, lds_f);
  float se = 0.f;
  for (int i = tid; i < a.V; i += 1024) se += expf(scaled(i) - m);
  const float z = block_sum<16>(se, lds_f);
  if (tid == 0) st.commit(b, t, f, (scaled(f) - m) - logf(z), 0.f, st.score_forced != 0);
}

// one draw: argmax(x + Gumbel noise) over the surviving set == multinomial(softmax(filtered)), then the step's bookkeeping
__global__ __launch_bounds__(1024) void sample_step_kernel(SampleArgs a, StepState st, int t) {
  __shared__ SampleLds lds;
  __shared__ float s_v[16], s_second[16];
  __shared__ int s_i[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (st.skip_finished(b, t)) return;
  const int f = st.forced_at(b, t, a.V);   // the same for every thread; the free rows of the launch draw what they always draw
  if (f >= 0) {
    sample_take_forced(a, st, b, t, f, lds.f);
    return;
  }
  float x[SM_NPT], m, z;
  uint32_t key[SM_NPT];
  const uint32_t thr = sample_filter(a, b, 1, x, key, m, z, lds);
  const uint32_t hrow = sample_stream(a, b, t);
  Pick<true, true> best;                   // runner-up for the margin; payload = the winner's unperturbed logit
#pragma unroll
  for (int j = 0; j < SM_NPT; ++j) {
    const int i = tid + j * 1024;
    if (key[j] >= thr) best.offer(gumbel_score(x[j], hrow, i), i, x[j]);
  }
  best = block_pick<16>(best, {s_v, s_i, s_second, lds.f});
  // log_softmax of the FILTERED, temperature-scaled logits
  if (tid == 0) st.commit(b, t, best.i, best.x - m - logf(z), best.v - best.second);
}

// The do_sample branch of beam search (modeling_utils.py:966-985): the same filter with min_tokens_to_keep = 2, then TWO draws
// without replacement (the two largest of x + Gumbel noise == torch.multinomial(p, 2)); written per row: the two words, their
// temperature-scaled logits and the log-sum-exp of the surviving set (so log_softmax(filtered)[word] = value - lse).
__global__ __launch_bounds__(1024) void beam_sample_kernel(SampleArgs a, int t, const int32_t* __restrict__ live,
                                                           float* __restrict__ cand_val, int32_t* __restrict__ cand_idx,
                                                           float* __restrict__ cand_lse) {
  VC_LIVE_EXIT(live);                      // every image's search has closed
  __shared__ SampleLds lds;
  __shared__ float s_v[16];
  __shared__ int s_i[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  float x[SM_NPT], m, z;
  uint32_t key[SM_NPT];
  const uint32_t thr = sample_filter(a, b, 2, x, key, m, z, lds);
  const uint32_t hrow = sample_stream(a, b, t);
  float sc[SM_NPT];
#pragma unroll
  for (int j = 0; j < SM_NPT; ++j) sc[j] = key[j] >= thr ? gumbel_score(x[j], hrow, tid + j * 1024) : -INFINITY;
  int excl = -1;
  for (int d = 0; d < 2; ++d) {            // the largest, then the largest of the rest
    Pick<false, true> best;
#pragma unroll
    for (int j = 0; j < SM_NPT; ++j) {
      const int i = tid + j * 1024;
      if (key[j] >= thr && i != excl) best.offer(sc[j], i, x[j]);
    }
    __syncthreads();
    best = block_pick<16>(best, {s_v, s_i, nullptr, lds.f});
    excl = best.i;
    if (tid == 0) {
      cand_val[(size_t)b * 2 + d] = best.x;
      cand_idx[(size_t)b * 2 + d] = best.i;
    }
  }
  if (tid == 0) cand_lse[b] = m + logf(z);
}

// sigmoid + top-k (k <= 64), one 1024-thread workgroup per row; each thread keeps up to 32 candidates as sortable 64-bit keys
// (tk_key, select.h: larger value first, lower index on ties -- torch.topk's CPU order) and its own running maximum, so a round is
// one workgroup-wide max over 1024 cached values behind ONE barrier and a 32-element rescan by the one thread whose candidate was
// taken (k rescans of every thread's 32 values behind two barriers were 122 us per batch of 64 rows).
constexpr int TK_PER_THREAD = 32;
__global__ __launch_bounds__(1024) void sigmoid_topk_kernel(const float* __restrict__ logits, int ldl, int V, int k,
                                                            float thresh, int64_t* __restrict__ out_ids,
                                                            float* __restrict__ out_prob,
                                                            int64_t* __restrict__ out_len) {
  __shared__ unsigned long long s_wmax[2][16];      // double-buffered by round: ONE barrier per round (a wave can be at most one round ahead)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = logits + (size_t)b * ldl;
  unsigned long long key[TK_PER_THREAD];
  unsigned long long tmax = 0ull;                                   // below every real key (sigmoid > 0 maps above 2^63)
#pragma unroll
  for (int j = 0; j < TK_PER_THREAD; ++j) {
    const int i = tid + j * 1024;
    key[j] = i < V ? tk_key(1.0f / (1.0f + expf(-row[i])), i) : 0ull;   // sigmoid in (0,1); 0 = absent / taken
    tmax = key[j] > tmax ? key[j] : tmax;
  }
  int nlen = 0;
  for (int r = 0; r < k; ++r) {
    const unsigned long long wm = wave_max_u64(tmax);
    if (lane == 0) s_wmax[r & 1][w] = wm;
    __syncthreads();
    unsigned long long best = s_wmax[r & 1][0];
#pragma unroll
    for (int q = 1; q < 16; ++q) {
      const unsigned long long c = s_wmax[r & 1][q];
      best = c > best ? c : best;
    }
    if (tid == 0) {
      const float pv = tk_val(best);
      out_ids[(size_t)b * k + r] = tk_idx(best);
      out_prob[(size_t)b * k + r] = pv;
      if (pv >= thresh) ++nlen;
    }
    if (tmax == best) {                 // keys are unique (they carry the index): exactly one thread owns the winner
      tmax = 0ull;
#pragma unroll
      for (int j = 0; j < TK_PER_THREAD; ++j) {
        if (key[j] == best) key[j] = 0ull;
        tmax = key[j] > tmax ? key[j] : tmax;
      }
    }
  }
  if (tid == 0) out_len[b] = nlen;
}


// ------------------------------------------------------------------------------------------------
// Beam search (a13, modeling_utils.py:888-1100).  Per step:
//   row_topk_lse_kernel : per sequence row, logsumexp over the vocabulary and its 2*beams largest logits
//                         (the top 2*beams of a row are the only candidates that row can contribute, because
//                         log_softmax + beam_score is a per-row constant shift);
//   beam_step_kernel    : one thread per image merges beams x 2*beams candidates, sorts them by total score and
//                         replays the reference's python candidate loop + BeamHypotheses (n_hyp = 1) on the device;
//   beam_reorder_kernel : gathers the text K/V cache rows of the chosen parent beams.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void row_topk_lse_kernel(const float* __restrict__ logits, int ldl, int V, int k,
                                                            float* __restrict__ out_val, int* __restrict__ out_idx,
                                                            float* __restrict__ out_lse, const int32_t* __restrict__ live) {
  VC_LIVE_EXIT(live);
  // Threshold selection -- three scans of the 32 register values per thread instead of 2 per extracted element (k rounds of
  // rescanning + removing made this kernel VALU-bound: 150-210 us for 1280 rows):
  //   1. every thread's maximum; the k largest of the 1024 thread maxima (cheap: one value per thread);
  //   2. T = the k-th of those.  Keys are unique, so exactly k threads own a key >= T and every key of the row's top k is
  //      >= T: all keys >= T (at most 32 per such thread, <= 32 k in total) go to a list in LDS;
  //   3. wave 0 orders the list's k best.
  constexpr int CAP = TK_PER_THREAD * 16;
  __shared__ unsigned long long s_cand[16][16];      // [wave][round], k <= 16
  __shared__ unsigned long long s_list[CAP];
  __shared__ unsigned long long s_thr;
  __shared__ float s_sum[16];
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = logits + (size_t)b * ldl;
  unsigned long long key[TK_PER_THREAD];
  unsigned long long tmax = 0ull;
#pragma unroll
  for (int j = 0; j < TK_PER_THREAD; ++j) {
    const int i = tid + j * 1024;
    key[j] = i < V ? tk_key(row[i], i) : 0ull;        // 0 = nothing here (below every real key)
    tmax = key[j] > tmax ? key[j] : tmax;
  }
  if (tid == 0) s_n = 0;
  unsigned long long mine[1] = {tmax};                // k best thread maxima of this wave
  wave_take_k(mine, k, [&](int r, unsigned long long best) { if (lane == 0) s_cand[w][r] = best; });
  __syncthreads();
  if (w == 0) {
    unsigned long long c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = lane + u * 64;
      c[u] = idx < 16 * k ? s_cand[idx / k][idx % k] : 0ull;
    }
    wave_take_k(c, k, [&](int r, unsigned long long best) {
      if (lane == 0 && r == 0) s_cand[0][0] = best;    // the row maximum (slot reused; everyone has read the candidates)
      if (lane == 0 && r == k - 1) s_thr = best;       // k-th largest thread maximum (0 when the row has fewer than k values)
    });
  }
  __syncthreads();
  const unsigned long long thr = s_thr;
  const float rowmax = tk_val(s_cand[0][0]);
  float se = 0.f;                                      // logsumexp with the row max
#pragma unroll
  for (int j = 0; j < TK_PER_THREAD; ++j) {
    if (tid + j * 1024 < V) se += expf(tk_val(key[j]) - rowmax);
    if (key[j] != 0ull && key[j] >= thr) {
      const int pos = atomicAdd(&s_n, 1);
      if (pos < CAP) s_list[pos] = key[j];
    }
  }
  const float tot = block_sum<16>(se, s_sum);         // its barrier also publishes the list
  if (w == 0) {
    const int n = s_n < CAP ? s_n : CAP;
    unsigned long long c[CAP / 64];
#pragma unroll
    for (int u = 0; u < CAP / 64; ++u) {
      const int idx = lane + u * 64;
      c[u] = idx < n ? s_list[idx] : 0ull;
    }
    wave_take_k(c, k, [&](int r, unsigned long long best) {
      if (lane == 0) {
        out_val[(size_t)b * k + r] = tk_val(best);
        out_idx[(size_t)b * k + r] = tk_idx(best);
      }
    });
    if (lane == 0) out_lse[b] = rowmax + logf(tot);
  }
}

// The same candidates from the vocabulary GEMM's row statistics (vitcap_gemm_desc.rowstat: per row and 32-column piece the
// maximum, its column and sum exp(x - max)) instead of from the 30522-wide rows.  With T = the k-th largest (piece maximum,
// column) key, every element of the row's top k has a key >= T and therefore lives in one of the k pieces whose maximum key
// is >= T (those k maxima are k distinct elements, so the k-th largest element is >= T): only k x 32 logits are read back.
// logsumexp = rowmax + log(sum_p se_p * exp(max_p - rowmax)).  One 256-thread workgroup per row.
__global__ __launch_bounds__(256) void row_topk_pieces_kernel(const float* __restrict__ logits, int ldl, int V,
                                                              const float* __restrict__ rowstat, int pieces, int k,
                                                              float* __restrict__ out_val, int* __restrict__ out_idx,
                                                              float* __restrict__ out_lse, const int32_t* __restrict__ live) {
  VC_LIVE_EXIT(live);
  constexpr int PPT = 4;                               // pieces per thread (956 pieces / 256 threads)
  __shared__ unsigned long long s_cand[4][16];
  __shared__ unsigned long long s_sel[16];             // the k largest piece keys, descending
  __shared__ unsigned long long s_list[512];           // k <= 16 pieces x 32 columns
  __shared__ float s_sum[4];
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const f32x4* rs = (const f32x4*)rowstat + (size_t)b * pieces;
  unsigned long long key[PPT], mine[PPT];
  float pm[PPT], ps[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = tid + j * 256;
    if (i < pieces) {
      const f32x4 r = rs[i];
      key[j] = tk_key(r[0], __float_as_int(r[1]));
      pm[j] = r[0];
      ps[j] = r[2];
    } else {
      key[j] = 0ull; pm[j] = -INFINITY; ps[j] = 0.f;
    }
    mine[j] = key[j];
  }
  if (tid == 0) s_n = 0;
  // the k best piece keys of this wave
  wave_take_k(mine, k, [&](int r, unsigned long long best) { if (lane == 0) s_cand[w][r] = best; });
  __syncthreads();
  if (w == 0) {
    unsigned long long c[1] = {lane < 4 * k ? s_cand[lane / k][lane % k] : 0ull};
    wave_take_k(c, k, [&](int r, unsigned long long best) { if (lane == 0) s_sel[r] = best; });
  }
  __syncthreads();
  const unsigned long long thr = s_sel[k - 1];
  const float rowmax = tk_val(s_sel[0]);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < PPT; ++j)
    if (ps[j] > 0.f) se += ps[j] * expf(pm[j] - rowmax);
  se = wave_sum(se);
  if (lane == 0) s_sum[w] = se;
  // the k selected pieces' 32 columns each: keep what is >= the threshold key
  for (int e = tid; e < k * 32; e += 256) {
    const unsigned long long sk = s_sel[e >> 5];
    if (sk == 0ull) continue;
    const int col = ((tk_idx(sk) >> 5) << 5) + (e & 31);
    if (col < V) {
      const unsigned long long kk = tk_key(logits[(size_t)b * ldl + col], col);
      if (kk >= thr) s_list[atomicAdd(&s_n, 1)] = kk;
    }
  }
  __syncthreads();
  if (w == 0) {
    const int n = s_n;
    unsigned long long c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = lane + u * 64;
      c[u] = idx < n ? s_list[idx] : 0ull;
    }
    wave_take_k(c, k, [&](int r, unsigned long long best) {
      if (lane == 0) {
        out_val[(size_t)b * k + r] = tk_val(best);
        out_idx[(size_t)b * k + r] = tk_idx(best);
      }
    });
    // this site adds its four wave partials pairwise, not serially (block_sum would change the last bit): kept as it is
    if (lane == 0) out_lse[b] = rowmax + logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
  }
}

constexpr int MAXBEAM = 8;

struct BeamState {
  int64_t* ids_in;      // [B*K][max_len]
  int64_t* ids_out;     // [B*K][max_len]
  float* beam_scores;   // [B*K]
  int* parent;          // [B*K]
  int* done;            // [B]
  int* has_hyp;         // [B]               number of hypotheses kept (0..n_keep)
  float* hyp_score;     // [B][n_keep]       in insertion order, like BeamHypotheses.hyp
  int* hyp_len;         // [B][n_keep]
  int64_t* hyp_tok;     // [B][n_keep][max_len]
  int n_keep;           // BeamHypotheses.n_hyp = num_keep_best
};

__global__ void beam_init_kernel(BeamState st, int B, int K, int max_len, int bos, int pad, int32_t* live) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && live) *live = B;     // images whose search is still open
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * K * max_len) {
    st.ids_in[i] = (i % max_len == 0) ? bos : pad;
    st.ids_out[i] = (i % max_len == 0) ? bos : pad;
  }
  if (i < B * K) {
    st.beam_scores[i] = (i % K == 0) ? 0.f : -1e9f;
    st.parent[i] = i;
  }
  if (i < B) {
    st.done[i] = 0;
    st.has_hyp[i] = 0;
  }
  if (i < B * st.n_keep) {
    st.hyp_score[i] = -1e30f;
    st.hyp_len[i] = 0;
  }
  if (i < B * st.n_keep * max_len) st.hyp_tok[i] = pad;
}

// One WAVE per image (before: one thread per image, ~150 dependent global accesses in series = 108 us per step at 256 images).
//   1. lanes load the beams x 2*beams candidates (score = value - lse + beam score, flat index = beam * V + word) into LDS;
//   2. every candidate computes its RANK under (score desc, flat index asc) against all others: rank r < 2*beams = position r
//      of the reference's sorted topk;
//   3. lane 0 replays the reference's candidate loop + BeamHypotheses on metadata only (scores, lengths, and for every kept
//      hypothesis WHERE its tokens come from: an old slot or a beam of this step);
//   4. all lanes materialise the token rows (hypotheses first read into registers, then written: slots may permute) and the
//      new beams' prefixes.
__global__ __launch_bounds__(64) void beam_step_kernel(const float* __restrict__ cval, const int* __restrict__ cidx,
                                                       const float* __restrict__ lse, BeamState st, int B, int K, int V, int t,
                                                       int max_len, int eos, int pad, float length_penalty, int32_t* __restrict__ live,
                                                       int sampled) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  // every image done (`if all(done): break`, modeling_utils.py:1072): beams, hypotheses and scores stay as they are
  if (live && *live == 0) return;
  const int C = 2 * K, n = sampled ? C : K * C, NH = st.n_keep;
  __shared__ float s_sc[MAXBEAM * 2 * MAXBEAM];
  __shared__ int s_fl[MAXBEAM * 2 * MAXBEAM];
  __shared__ float s_top_sc[2 * MAXBEAM];
  __shared__ int s_top_fl[2 * MAXBEAM];
  __shared__ float s_hsc[MAXBEAM];       // kept hypotheses after this step
  __shared__ int s_hln[MAXBEAM];
  __shared__ int s_hsrc[MAXBEAM];        // >= 0: old slot; < 0: -(1 + beam) of this step
  __shared__ int s_nh;
  __shared__ float s_nsc[MAXBEAM];
  __shared__ int s_nword[MAXBEAM], s_npar[MAXBEAM];
  __shared__ float s_best_sc;
  if (sampled) {
    // do_sample (modeling_utils.py:966-985): the candidates are the 2 draws of each beam IN POSITION ORDER, not ranked.
    // Position p holds draw p % 2 of beam p / 2 (score = its log-prob + THAT beam's score), but the reference's "match shape of
    // greedy beam search" step adds `arange(K) * V` repeated twice as beam offsets, so position p is ATTRIBUTED to beam p % K:
    // the prefix continued (or finished) with the word is beam p % K's.  Reproduced as written.
    for (int i = lane; i < n; i += 64) {
      const int row = b * K + (i >> 1);
      s_top_sc[i] = cval[(size_t)row * 2 + (i & 1)] + (st.beam_scores[row] - lse[row]);
      s_top_fl[i] = (i % K) * V + cidx[(size_t)row * 2 + (i & 1)];
    }
    __syncthreads();
    if (lane == 0) {
      float mx = s_top_sc[0];
      for (int i = 1; i < n; ++i) mx = fmaxf(mx, s_top_sc[i]);
      s_best_sc = mx;                                          // is_done(next_scores.max())
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const int k = i / C, row = b * K + k;
      s_sc[i] = cval[(size_t)row * C + (i - k * C)] + (st.beam_scores[row] - lse[row]);   // log_softmax + beam score
      s_fl[i] = k * V + cidx[(size_t)row * C + (i - k * C)];                              // index into the (beams*V) view
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
      const float v = s_sc[i];
      const int f = s_fl[i];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (s_sc[j] > v || (s_sc[j] == v && s_fl[j] < f)) ? 1 : 0;
      if (rank < C) { s_top_sc[rank] = v; s_top_fl[rank] = f; }
      if (rank == 0) s_best_sc = v;
    }
  }
  float* hsc = st.hyp_score + (size_t)b * NH;
  int* hln = st.hyp_len + (size_t)b * NH;
  int64_t* htk = st.hyp_tok + (size_t)b * NH * max_len;
  // old hypothesis rows into registers (NH * max_len <= 8 * 40 = 320 values, <= 5 per lane)
  int64_t old_tok[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int i = lane + u * 64;
    old_tok[u] = i < NH * max_len ? htk[i] : 0;
  }
  __syncthreads();
  if (lane == 0) {
    int nh = st.has_hyp[b];
    for (int i = 0; i < nh; ++i) { s_hsc[i] = hsc[i]; s_hln[i] = hln[i]; s_hsrc[i] = i; }
    int done = st.done[b];
    const int was_done = done;
    if (!done && nh >= NH) {
      // BeamHypotheses.is_done: the list is full and its worst score already beats what the best open beam can reach
      float worst = s_hsc[0];
      for (int i = 1; i < nh; ++i) worst = fminf(worst, s_hsc[i]);
      if (worst >= s_best_sc / powf((float)(max_len - 1), length_penalty)) done = 1;
    }
    int cnt = 0;
    if (!done) {
      const bool last = (t + 1 == max_len);
      for (int r = 0; r < C && cnt < K; ++r) {
        const int beam = s_top_fl[r] / V, word = s_top_fl[r] - beam * V;
        if (word == eos || last) {
          // BeamHypotheses.add (modeling_utils.py:1157-1170): append when the list is not full or the score beats the worst
          // kept one; when that makes n_hyp + 1 entries, delete the lowest (first of equals) and keep the insertion order
          const float hs = s_top_sc[r] / powf((float)t, length_penalty);     // len(hyp) == cur_len == t
          int slot = -1;
          if (nh < NH) {
            slot = nh++;
          } else {
            int lo = 0;
            for (int i = 1; i < nh; ++i)
              if (s_hsc[i] < s_hsc[lo]) lo = i;
            if (hs > s_hsc[lo]) {
              for (int i = lo; i + 1 < nh; ++i) { s_hsc[i] = s_hsc[i + 1]; s_hln[i] = s_hln[i + 1]; s_hsrc[i] = s_hsrc[i + 1]; }
              slot = nh - 1;
            }
          }
          if (slot >= 0) { s_hsc[slot] = hs; s_hln[slot] = t; s_hsrc[slot] = -(1 + beam); }
        } else {
          s_nsc[cnt] = s_top_sc[r];
          s_nword[cnt] = word;
          s_npar[cnt] = b * K + beam;
          ++cnt;
        }
      }
    }
    if (cnt < K) {   // finished image (or the last step): filler beams, ignored from here on
      for (int i = 0; i < K; ++i) { s_nsc[i] = 0.f; s_nword[i] = pad; s_npar[i] = b * K; }
    }
    s_nh = nh;
    if (live && done && !was_done) atomicSub(live, 1);
    st.done[b] = done;
    st.has_hyp[b] = nh;
    for (int i = 0; i < nh; ++i) { hsc[i] = s_hsc[i]; hln[i] = s_hln[i]; }
  }
  __syncthreads();
  // hypothesis token rows: slot i <- old slot s_hsrc[i] (from the registers, via LDS exchange) or beam -(s_hsrc[i]+1)'s prefix
  __shared__ int64_t s_old[MAXBEAM * 40];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int i = lane + u * 64;
    if (i < NH * max_len && i < MAXBEAM * 40) s_old[i] = old_tok[u];
  }
  __syncthreads();
  const int nh = s_nh;
  for (int i = lane; i < nh * max_len; i += 64) {
    const int slot = i / max_len, q = i - slot * max_len;
    const int src = s_hsrc[slot];
    int64_t v;
    if (src >= 0) v = s_old[src * max_len + q];
    else v = q < t ? st.ids_in[(size_t)(b * K + (-src - 1)) * max_len + q] : (int64_t)pad;
    htk[i] = v;
  }
  // the K beams leaving the step: parent prefix + the chosen word
  for (int i = lane; i < K * (t + 1); i += 64) {
    const int k = i / (t + 1), q = i - k * (t + 1);
    st.ids_out[(size_t)(b * K + k) * max_len + q] = q < t ? st.ids_in[(size_t)s_npar[k] * max_len + q] : (int64_t)s_nword[k];
  }
  if (lane < K) {
    st.beam_scores[b * K + lane] = s_nsc[lane];
    st.parent[b * K + lane] = s_npar[lane];
  }
}

// dst[l][s][0..t) = src[l][parent[s]][0..t)   (rows of 2*768 bf16 = 3 KiB)
__global__ __launch_bounds__(192) void beam_reorder_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                           const int* __restrict__ parent, int NS, int max_len, int t,
                                                           const int32_t* __restrict__ live) {
  VC_LIVE_EXIT(live);
  const int s = blockIdx.x, l = blockIdx.y;
  const size_t rowv = 2 * 768 * 2 / 16;   // 192 uint4 per position
  const uint4* sp = src + ((size_t)l * NS + parent[s]) * max_len * rowv;
  uint4* dp = dst + ((size_t)l * NS + s) * max_len * rowv;
  for (int q = 0; q < t; ++q) dp[q * rowv + threadIdx.x] = sp[q * rowv + threadIdx.x];
}

// decoded[b][j] = the j-th best kept hypothesis + EOS, padded; logprobs -1e5 where fewer than n_keep finished
// (modeling_utils.py:1076-1100: topk over the kept scores, best first; equal scores: earlier insertion first)
__global__ void beam_finalize_kernel(BeamState st, int64_t* out_ids, float* out_lp, int B, int max_len, int eos, int pad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int NH = st.n_keep, nh = st.has_hyp[b];
  const float* hsc = st.hyp_score + (size_t)b * NH;
  unsigned used = 0;
  for (int j = 0; j < NH; ++j) {
    int best = -1;
    for (int i = 0; i < nh; ++i)
      if (!(used >> i & 1) && (best < 0 || hsc[i] > hsc[best])) best = i;
    int64_t* dst = out_ids + ((size_t)b * NH + j) * max_len;
    if (best < 0) {
      for (int i = 0; i < max_len; ++i) dst[i] = pad;
      out_lp[(size_t)b * NH + j] = -1e5f;
      continue;
    }
    used |= 1u << best;
    const int Lh = st.hyp_len[(size_t)b * NH + best];
    const int64_t* src = st.hyp_tok + ((size_t)b * NH + best) * max_len;
    for (int i = 0; i < max_len; ++i) dst[i] = i < Lh ? src[i] : (i == Lh ? (int64_t)eos : (int64_t)pad);
    out_lp[(size_t)b * NH + j] = hsc[best];
  }
}

// CTRL repetition penalty as generate() applies it (modeling_utils.py:828-836 greedy / sampling, 955-963 beam): for every
// DISTINCT token already in the sequence (`set(input_ids[i].tolist())`, [CLS] included), logit < 0 ? logit * p : logit / p.
// One wave per row; lane j owns prefix position j and acts if no earlier position holds the same token.
__global__ __launch_bounds__(256) void repetition_penalty_kernel(float* __restrict__ logits, int ldl, int V,
                                                                 const int64_t* __restrict__ ids, int ld_ids, int t,
                                                                 float penalty, int rows, const int32_t* __restrict__ live) {
  VC_LIVE_EXIT(live);
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || lane >= t) return;
  const int64_t* r = ids + (size_t)row * ld_ids;
  const int64_t tok = r[lane];
  for (int j = 0; j < lane; ++j)
    if (r[j] == tok) return;
  if (tok < 0 || tok >= V) return;
  float* x = logits + (size_t)row * ldl + tok;
  const float v = *x;
  *x = v < 0.f ? v * penalty : v / penalty;
}

// ---- one-pass caption scoring (vitcap_score_rows, include/vitcap_hip.h) -------------------------------------------------------
// Probe row g of the grid = caption g / (L-1), position t = g % (L-1) + 1.  One 1024-thread workgroup per row, the reductions of
// greedy_step_kernel; every row decides on its own whether its caption has ended before it (its ids are all known), so a launch
// may cover any range of rows.  The row's rules live in score_row.h, shared with the alternatives kernel.
__global__ __launch_bounds__(1024) void score_rows_kernel(const float* __restrict__ logits, int ldl, int V, ScoreArgs a, int rows0) {
  __shared__ float s_v[16], s_sum[16];
  __shared__ int s_i[16];
  const int tid = threadIdx.x;
  int b, t;
  score_row_place(rows0 + blockIdx.x, a.L, b, t);
  const int64_t* cap = a.ids + (size_t)b * a.L;
  if (score_row_ended(cap, t, a.eos, a.eos_x)) {      // behind the end: nothing is counted
    if (tid == 0) score_row_write_dead(a, b, t);
    return;
  }
  const float* row = logits + (size_t)blockIdx.x * ldl;
  Pick<false, false> best;
  for (int i = tid; i < V; i += 1024) best.offer(row[i], i);
  best = block_pick<16>(best, {s_v, s_i, nullptr, nullptr});
  float se = 0.f;
  for (int i = tid; i < V; i += 1024) se += score_row_term(row[i], best.v);
  const float tot = block_sum<16>(se, s_sum);
  if (tid != 0) return;
  const int f = score_row_token(cap, a.last_tok, b, t, a.L, a.eos, V, best.i);
  score_row_write(a, b, t, f, score_row_lp(row[f], best.v, tot));
}
// the captions whose last probe row lies in [rows0, rows0 + n_rows): their sums, taken in position order like the step loop's
__global__ void score_finish_kernel(ScoreArgs a, int n_caps, int rows0, int n_rows) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_caps) return;
  const long long lastrow = (long long)b * (a.L - 1) + (a.L - 2);
  if (lastrow < rows0 || lastrow >= (long long)rows0 + n_rows) return;
  const int64_t* cap = a.ids + (size_t)b * a.L;
  float s = 0.f, c = 0.f;
  for (int t = 1; t < a.L; ++t) {
    s += a.tok_lp[(size_t)b * a.L + t];
    c += 1.0f;
    if (vc_is_eos((int)cap[t], a.eos, a.eos_x)) break;
  }
  a.tok_lp[(size_t)b * a.L] = 0.f;
  a.out_ids[(size_t)b * a.L] = cap[0];
  if (a.sum_lp) a.sum_lp[b] = s;
  if (a.cnt) a.cnt[b] = c;
  a.logprob[b] = StepState::mean_lp(s, c);
}
// the grid's token ids for vitcap_embed_rows: [n_caps][2L-1] = the caption's L tokens, then L-1 [MASK]
__global__ void score_grid_ids_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ grid, int n_caps, int L, int mask, int pad,
                                      int V) {
  const int R = 2 * L - 1;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_caps * R) return;
  const int b = (int)(i / R), r = (int)(i - (long long)b * R);
  int64_t tok = mask;
  if (r < L) {
    tok = ids[(size_t)b * L + r];
    if (tok < 0 || tok >= (int64_t)V) tok = pad;      // never an index outside the embedding table
  }
  grid[i] = tok;
}

}  // namespace

int vc_score_grid_ids(const int64_t* ids, int64_t* grid, int n_caps, int L, int mask, int pad, void* stream) {
  VC_REQUIRE(ids && grid && n_caps > 0 && L >= 2, "score_grid_ids: bad arguments");
  const long long n = (long long)n_caps * (2 * L - 1);
  hipLaunchKernelGGL(score_grid_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids, grid, n_caps, L, mask,
                     pad, VITCAP_VOCAB);
  VC_LAUNCH_CHECK("score_grid_ids");
  return VITCAP_OK;
}

int vc_score_finish(const ScoreArgs& a, int n_caps, int rows0, int n_rows, void* stream) {
  hipLaunchKernelGGL(score_finish_kernel, dim3((n_caps + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, n_caps, rows0, n_rows);
  VC_LAUNCH_CHECK("score_rows (sums)");
  return VITCAP_OK;
}

extern "C" int vitcap_score_rows(const float* logits, int ldl, int V, const int64_t* caption_ids, const int64_t* last_tok, int rows0,
                                 int n_rows, int n_caps, int max_len, int eos, const int32_t* eos_extra, int pad, float* sum_lp,
                                 float* cnt, float* token_logprobs, int64_t* out_ids, int64_t* out_last_tok, float* logprob_out,
                                 void* stream) {
  VC_REQUIRE(logits && caption_ids && token_logprobs && out_ids && logprob_out, "score_rows: null pointer");
  VC_REQUIRE(V > 0 && ldl >= V && n_caps > 0 && max_len >= 2 && max_len <= 40, "score_rows: bad sizes (max_len=%d)", max_len);
  VC_REQUIRE(rows0 >= 0 && n_rows > 0 && (long long)rows0 + n_rows <= (long long)n_caps * (max_len - 1),
             "score_rows: rows [%d, %d + %d) outside the %d x %d probe rows", rows0, rows0, n_rows, n_caps, max_len - 1);
  ScoreArgs a{caption_ids, last_tok, token_logprobs, out_ids, out_last_tok, sum_lp, cnt, logprob_out, max_len, eos, pad,
              VcEosExtra{{eos_extra ? eos_extra[0] : -1, eos_extra ? eos_extra[1] : -1, eos_extra ? eos_extra[2] : -1}}};
  hipLaunchKernelGGL(score_rows_kernel, dim3(n_rows), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V, a, rows0);
  VC_LAUNCH_CHECK("score_rows");
  return vc_score_finish(a, n_caps, rows0, n_rows, stream);
}

extern "C" int vitcap_repetition_penalty(float* logits, int ldl, int V, const int64_t* ids, int ld_ids, int t, float penalty,
                                         int rows, void* stream) {
  VC_REQUIRE(logits && ids && rows > 0 && V > 0 && ldl >= V && t >= 1 && t <= ld_ids && t <= 64 && penalty > 0.f,
             "repetition_penalty: bad arguments (t=%d, penalty=%g)", t, (double)penalty);
  hipLaunchKernelGGL(repetition_penalty_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, ids,
                     ld_ids, t, penalty, rows, vc_tls_live);
  VC_LAUNCH_CHECK("repetition_penalty");
  return VITCAP_OK;
}

extern "C" int vitcap_greedy_init(int64_t* ids, int32_t* unfinished, float* sum_lp, float* cnt, int B, int max_len,
                                  int bos, int pad, void* stream) {
  VC_REQUIRE(ids && unfinished && sum_lp && cnt && B > 0 && max_len > 1, "greedy_init: bad arguments");
  const int n = B * max_len;
  hipLaunchKernelGGL(greedy_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, unfinished,
                     sum_lp, cnt, B, max_len, bos, pad, (int32_t*)vc_tls_live);
  VC_LAUNCH_CHECK("greedy_init");
  return VITCAP_OK;
}

extern "C" int vitcap_greedy_step_forced(const float* logits, int ldl, int V, int64_t* ids, int32_t* unfinished,
                                         float* sum_lp, float* cnt, float* logprob_out, float* margin_out, int64_t* raw_last,
                                         int B, int t, int max_len, int eos, int pad, const int64_t* forced_ids, int score_forced,
                                         float* token_logprobs, void* stream) {
  VC_REQUIRE(logits && ids && unfinished && sum_lp && cnt && logprob_out, "greedy_step: null pointer");
  VC_REQUIRE(B > 0 && V > 0 && ldl >= V && t >= 1 && t < max_len, "greedy_step: bad sizes (t=%d)", t);
  VC_REQUIRE(score_forced == 0 || score_forced == 1, "greedy_step: score_forced must be 0 or 1 (got %d)", score_forced);
  hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V,
                     vc_step_state(ids, unfinished, sum_lp, cnt, logprob_out, raw_last, margin_out, max_len, eos, pad, forced_ids,
                                   score_forced, token_logprobs), t);
  VC_LAUNCH_CHECK("greedy_step");
  return VITCAP_OK;
}

extern "C" int vitcap_greedy_step(const float* logits, int ldl, int V, int64_t* ids, int32_t* unfinished,
                                  float* sum_lp, float* cnt, float* logprob_out, float* margin_out, int64_t* raw_last,
                                  int B, int t, int max_len, int eos, int pad, void* stream) {
  return vitcap_greedy_step_forced(logits, ldl, V, ids, unfinished, sum_lp, cnt, logprob_out, margin_out, raw_last, B, t, max_len, eos,
                                   pad, nullptr, 0, nullptr, stream);
}

extern "C" int vitcap_sigmoid_topk(const float* logits, int ldl, int V, int k, float thresh, int64_t* out_ids,
                                   float* out_prob, int64_t* out_len, int B, void* stream) {
  VC_REQUIRE(logits && out_ids && out_prob && out_len && B > 0, "sigmoid_topk: bad arguments");
  VC_REQUIRE(k >= 1 && k <= 64 && V <= TK_PER_THREAD * 1024 && ldl >= V, "sigmoid_topk: k=%d V=%d unsupported", k, V);
  hipLaunchKernelGGL(sigmoid_topk_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V, k, thresh,
                     out_ids, out_prob, out_len);
  VC_LAUNCH_CHECK("sigmoid_topk");
  return VITCAP_OK;
}


extern "C" int vitcap_row_topk_lse(const float* logits, int ldl, int V, int k, float* out_val, int32_t* out_idx,
                                   float* out_lse, int rows, void* stream) {
  VC_REQUIRE(logits && out_val && out_idx && out_lse && rows > 0, "row_topk_lse: bad arguments");
  VC_REQUIRE(k >= 1 && k <= 16 && V <= TK_PER_THREAD * 1024 && ldl >= V, "row_topk_lse: k=%d V=%d unsupported", k, V);
  hipLaunchKernelGGL(row_topk_lse_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, logits, ldl, V, k, out_val,
                     out_idx, out_lse, vc_tls_live);
  VC_LAUNCH_CHECK("row_topk_lse");
  return VITCAP_OK;
}

extern "C" int vitcap_row_topk_pieces(const float* logits, int ldl, int V, const float* rowstat, int pieces, int k,
                                      float* out_val, int32_t* out_idx, float* out_lse, int rows, void* stream) {
  VC_REQUIRE(logits && rowstat && out_val && out_idx && out_lse && rows > 0, "row_topk_pieces: bad arguments");
  VC_REQUIRE(k >= 1 && k <= 16 && ldl >= V && pieces >= k && pieces <= 1024 && pieces * 32 >= V,
             "row_topk_pieces: k=%d V=%d pieces=%d unsupported", k, V, pieces);
  hipLaunchKernelGGL(row_topk_pieces_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, rowstat, pieces, k,
                     out_val, out_idx, out_lse, vc_tls_live);
  VC_LAUNCH_CHECK("row_topk_pieces");
  return VITCAP_OK;
}

static BeamState make_state(const vitcap_beam_state* s) {
  BeamState st;
  st.ids_in = s->ids_in; st.ids_out = s->ids_out; st.beam_scores = s->beam_scores; st.parent = s->parent;
  st.done = s->done; st.has_hyp = s->has_hyp; st.hyp_score = s->hyp_score; st.hyp_len = s->hyp_len;
  st.hyp_tok = s->hyp_tok;
  st.n_keep = s->n_keep;
  return st;
}

extern "C" int vitcap_beam_init(const vitcap_beam_state* s, int B, int K, int max_len, int bos, int pad, void* stream) {
  VC_REQUIRE(s && B > 0 && K >= 1 && K <= MAXBEAM && max_len > 1, "beam_init: bad arguments (beams <= %d)", MAXBEAM);
  VC_REQUIRE(s->n_keep >= 1 && s->n_keep <= MAXBEAM, "beam_init: n_keep must be 1..%d (got %d)", MAXBEAM, s->n_keep);
  const int n = B * (K > s->n_keep ? K : s->n_keep) * max_len;
  hipLaunchKernelGGL(beam_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, make_state(s), B, K,
                     max_len, bos, pad, (int32_t*)vc_tls_live);
  VC_LAUNCH_CHECK("beam_init");
  return VITCAP_OK;
}

// `who` = the entry point's name in the error texts; sampled candidates need two beams
static int launch_beam_step(const char* who, int sampled, const float* cand_val, const int32_t* cand_idx, const float* lse,
                            const vitcap_beam_state* s, int B, int K, int V, int t, int max_len, int eos, int pad,
                            float length_penalty, void* stream) {
  VC_REQUIRE(cand_val && cand_idx && lse && s && B > 0 && K >= (sampled ? 2 : 1) && K <= MAXBEAM, "%s: bad arguments", who);
  VC_REQUIRE(t >= 1 && t < max_len && max_len <= 40, "%s: t=%d out of range (max_len %d <= 40)", who, t, max_len);
  VC_REQUIRE(s->n_keep >= 1 && s->n_keep <= MAXBEAM, "%s: n_keep must be 1..%d (got %d)", who, MAXBEAM, s->n_keep);
  hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cand_val, cand_idx, lse,
                     make_state(s), B, K, V, t, max_len, eos, pad, length_penalty, (int32_t*)vc_tls_live, sampled);
  VC_LAUNCH_CHECK(who);
  return VITCAP_OK;
}

extern "C" int vitcap_beam_step(const float* cand_val, const int32_t* cand_idx, const float* lse,
                                const vitcap_beam_state* s, int B, int K, int V, int t, int max_len, int eos, int pad,
                                float length_penalty, void* stream) {
  return launch_beam_step("beam_step", 0, cand_val, cand_idx, lse, s, B, K, V, t, max_len, eos, pad, length_penalty, stream);
}

// The same step on SAMPLED candidates (vitcap_beam_sample_candidates: cand_val / cand_idx [B*K][2], lse [B*K]): consumed in
// position order with the reference's beam attribution (see beam_step_kernel).
extern "C" int vitcap_beam_step_sampled(const float* cand_val, const int32_t* cand_idx, const float* lse,
                                        const vitcap_beam_state* s, int B, int K, int V, int t, int max_len, int eos, int pad,
                                        float length_penalty, void* stream) {
  return launch_beam_step("beam_step_sampled", 1, cand_val, cand_idx, lse, s, B, K, V, t, max_len, eos, pad, length_penalty, stream);
}

extern "C" int vitcap_beam_reorder_cache(const void* src, void* dst, const int32_t* parent, int layers, int NS,
                                         int max_len, int t, void* stream) {
  VC_REQUIRE(src && dst && parent && layers > 0 && NS > 0 && t >= 1 && t <= max_len, "beam_reorder: bad arguments");
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(NS, layers), dim3(192), 0, (hipStream_t)stream, (const uint4*)src,
                     (uint4*)dst, parent, NS, max_len, t, vc_tls_live);
  VC_LAUNCH_CHECK("beam_reorder");
  return VITCAP_OK;
}

extern "C" int vitcap_beam_finalize(const vitcap_beam_state* s, int64_t* out_ids, float* out_logprobs, int B,
                                    int max_len, int eos, int pad, void* stream) {
  VC_REQUIRE(s && out_ids && out_logprobs && B > 0, "beam_finalize: bad arguments");
  VC_REQUIRE(s->n_keep >= 1 && s->n_keep <= MAXBEAM, "beam_finalize: n_keep must be 1..%d (got %d)", MAXBEAM, s->n_keep);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, make_state(s),
                     out_ids, out_logprobs, B, max_len, eos, pad);
  VC_LAUNCH_CHECK("beam_finalize");
  return VITCAP_OK;
}

static int check_sample_params(const char* who, const vitcap_sample_params* sp) {
  VC_REQUIRE(sp->temperature > 0.f && sp->top_k >= 0 && sp->top_p > 0.f, "%s: temperature %g / top_k %d / top_p %g out of range", who,
             (double)sp->temperature, sp->top_k, (double)sp->top_p);
  return VITCAP_OK;
}
static SampleArgs sample_args(const float* logits, int ldl, int V, const vitcap_sample_params* sp, int seq_offset) {
  return SampleArgs{logits, ldl, V, sp->temperature, sp->top_k, sp->top_p, sp->seed, seq_offset};
}

extern "C" int vitcap_sample_step_forced(const float* logits, int ldl, int V, int64_t* ids, int32_t* unfinished,
                                         float* sum_lp, float* cnt, float* logprob_out, float* margin_out, int64_t* raw_last,
                                         int B, int t, int max_len, int eos, int pad, const vitcap_sample_params* sp, int seq_offset,
                                         const int64_t* forced_ids, int score_forced, float* token_logprobs, void* stream) {
  VC_REQUIRE(logits && ids && unfinished && sum_lp && cnt && logprob_out && sp, "sample_step: null pointer");
  VC_REQUIRE(B > 0 && V > 0 && V <= SM_NPT * 1024 && ldl >= V && t >= 1 && t < max_len && seq_offset >= 0,
             "sample_step: bad sizes (V=%d t=%d)", V, t);
  VC_REQUIRE(score_forced == 0 || score_forced == 1, "sample_step: score_forced must be 0 or 1 (got %d)", score_forced);
  if (const int rc = check_sample_params("sample_step", sp)) return rc;
  hipLaunchKernelGGL(sample_step_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, sample_args(logits, ldl, V, sp, seq_offset),
                     vc_step_state(ids, unfinished, sum_lp, cnt, logprob_out, raw_last, margin_out, max_len, eos, pad, forced_ids,
                                   score_forced, token_logprobs), t);
  VC_LAUNCH_CHECK("sample_step");
  return VITCAP_OK;
}

extern "C" int vitcap_sample_step_offset(const float* logits, int ldl, int V, int64_t* ids, int32_t* unfinished,
                                         float* sum_lp, float* cnt, float* logprob_out, float* margin_out, int64_t* raw_last,
                                         int B, int t, int max_len, int eos, int pad, const vitcap_sample_params* sp, int seq_offset,
                                         void* stream) {
  return vitcap_sample_step_forced(logits, ldl, V, ids, unfinished, sum_lp, cnt, logprob_out, margin_out, raw_last, B, t, max_len, eos,
                                   pad, sp, seq_offset, nullptr, 0, nullptr, stream);
}

extern "C" int vitcap_sample_step(const float* logits, int ldl, int V, int64_t* ids, int32_t* unfinished,
                                  float* sum_lp, float* cnt, float* logprob_out, float* margin_out, int64_t* raw_last,
                                  int B, int t, int max_len, int eos, int pad, const vitcap_sample_params* sp, void* stream) {
  return vitcap_sample_step_offset(logits, ldl, V, ids, unfinished, sum_lp, cnt, logprob_out, margin_out, raw_last, B, t, max_len, eos,
                                   pad, sp, 0, stream);
}

// Candidates of one beam-search step WITH sampling (modeling_utils.py:966-985): per row (= beam) two words drawn without
// replacement from softmax(filter(logits / temperature)), filter with min_tokens_to_keep = 2.  out_val / out_idx: [rows][2],
// out_lse: [rows]; vitcap_beam_step_sampled consumes them.  The noise stream of row r is (seed, r + row_offset, t).
extern "C" int vitcap_beam_sample_candidates(const float* logits, int ldl, int V, int rows, int t,
                                             const vitcap_sample_params* sp, int row_offset, float* out_val, int32_t* out_idx,
                                             float* out_lse, void* stream) {
  VC_REQUIRE(logits && sp && out_val && out_idx && out_lse, "beam_sample_candidates: null pointer");
  VC_REQUIRE(rows > 0 && V > 2 && V <= SM_NPT * 1024 && ldl >= V && t >= 1 && row_offset >= 0,
             "beam_sample_candidates: bad sizes (V=%d t=%d)", V, t);
  if (const int rc = check_sample_params("beam_sample_candidates", sp)) return rc;
  hipLaunchKernelGGL(beam_sample_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, sample_args(logits, ldl, V, sp, row_offset),
                     t, vc_tls_live, out_val, out_idx, out_lse);
  VC_LAUNCH_CHECK("beam_sample_candidates");
  return VITCAP_OK;
}
