// Row selection on the device, stated once: ordered keys, the argmax candidate, workgroup sum / max, "a wave takes the k best",
// radix selection, and the per-sequence bookkeeping of one generation step.  Used by decode.hip, norm.hip and cbs.hip (the keys).
//
// Floating-point sums keep one order: xor butterfly 32 -> 1 inside a wave (wave_sum), then the wave partials added serially
// 0 -> NW-1 (block_sum).  One site does NOT use block_sum and must keep its own expression, because its results are pinned bit
// for bit: row_topk_pieces_kernel (decode.hip) adds its four partials pairwise, (s0 + s1) + (s2 + s3).  Key, integer and max
// reductions do not depend on the order.
#pragma once
#include "common.h"
#include "call_state.h"   // vc_tls_live, vc_tls_eos_extra: read by the host helper vc_step_state at the end of this file

// ---- ordered keys ------------------------------------------------------------------------------------------------------
// float -> unsigned with unsigned order == float order, and back
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// (value, index) as ONE sortable 64-bit key: high word = the ordered value, low word = ~index, so "larger value first, lower
// index on ties" (torch.topk on CPU) is a plain unsigned max -- one compare per element instead of a two-field comparison.
// Keys are unique (they carry the index); 0 is below every real key and marks an empty slot.
__device__ __forceinline__ unsigned long long tk_key(float f, int i) {
  return ((unsigned long long)order_key(f) << 32) | (unsigned)(~i);
}
__device__ __forceinline__ float tk_val(unsigned long long k) { return order_val((uint32_t)(k >> 32)); }
__device__ __forceinline__ int tk_idx(unsigned long long k) { return (int)(~(unsigned)k); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)a, o, 64), hi = __shfl_xor((unsigned)(a >> 32), o, 64);
    const unsigned long long b = ((unsigned long long)hi << 32) | lo;
    a = b > a ? b : a;
  }
  return a;
}

// One wave takes the k best of the keys its lanes hold in c[N], best first.  emit(r, key) runs on every lane with round r's
// winner (0 once the keys have run out); the winner's slot is emptied.
template <int N, typename Emit>
__device__ __forceinline__ void wave_take_k(unsigned long long (&c)[N], int k, Emit emit) {
  for (int r = 0; r < k; ++r) {
    unsigned long long best = c[0];
#pragma unroll
    for (int u = 1; u < N; ++u) best = c[u] > best ? c[u] : best;
    best = wave_max_u64(best);
    emit(r, best);
#pragma unroll
    for (int u = 0; u < N; ++u)
      if (c[u] == best) c[u] = 0ull;
  }
}

// ---- workgroup sum / max of NW waves, result in every thread -------------------------------------------------------------
// s: NW floats of LDS; the trailing barrier frees them for their next use.  Four partials are in flight at a time: the sampling
// kernels hold a whole row in registers and have none to spare for sixteen.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* s) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float tot = 0.f;
#pragma unroll 4
  for (int k = 0; k < NW; ++k) tot += s[k];
  __syncthreads();
  return tot;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* s) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = s[0];
#pragma unroll 4
  for (int k = 1; k < NW; ++k) m = fmaxf(m, s[k]);
  __syncthreads();
  return m;
}

// ---- argmax candidate ------------------------------------------------------------------------------------------------------
// Value and index; with SECOND the runner-up value (the top-2 margin), with PAYLOAD a value that travels with the winner (the
// unperturbed logit of a noisy score).  Larger value wins; on ties the LOWER index wins (torch.argmax / topk on CPU).  Fields a
// caller does not ask for are never read: they cost neither registers, shuffles nor LDS.
template <bool SECOND, bool PAYLOAD>
struct Pick {
  float v = -INFINITY;
  int i = 0x7fffffff;
  float second = -INFINITY;
  float x = 0.f;
  __device__ __forceinline__ bool loses_to(float ov, int oi) const { return ov > v || (ov == v && oi < i); }
  // one more element / another candidate: the loser of the two bests becomes a runner-up candidate
  __device__ __forceinline__ void offer(float ov, int oi, float ox = 0.f) {
    const bool take = loses_to(ov, oi);
    if constexpr (SECOND) second = fmaxf(second, take ? v : ov);
    if constexpr (PAYLOAD) x = take ? ox : x;
    v = take ? ov : v;
    i = take ? oi : i;
  }
  __device__ __forceinline__ void merge(const Pick& o) {
    if constexpr (SECOND) second = fmaxf(second, o.second);
    offer(o.v, o.i, o.x);
  }
};
template <bool SECOND, bool PAYLOAD>
__device__ __forceinline__ Pick<SECOND, PAYLOAD> wave_pick(Pick<SECOND, PAYLOAD> a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Pick<SECOND, PAYLOAD> b;
    b.v = __shfl_xor(a.v, o, 64);
    b.i = __shfl_xor(a.i, o, 64);
    if constexpr (SECOND) b.second = __shfl_xor(a.second, o, 64);
    if constexpr (PAYLOAD) b.x = __shfl_xor(a.x, o, 64);
    a.merge(b);
  }
  return a;
}
// LDS of the workgroup reduction: NW entries each; second / x may be null when the candidate does not carry them
struct PickLds {
  float* v;
  int* i;
  float* second;
  float* x;
};
// Workgroup argmax of NW waves, result in every thread.  One barrier; the caller puts one between two uses of the same LDS.
template <int NW, bool SECOND, bool PAYLOAD>
__device__ __forceinline__ Pick<SECOND, PAYLOAD> block_pick(Pick<SECOND, PAYLOAD> a, PickLds s) {
  const int w = threadIdx.x >> 6;
  a = wave_pick(a);
  if ((threadIdx.x & 63) == 0) {
    s.v[w] = a.v;
    s.i[w] = a.i;
    if constexpr (SECOND) s.second[w] = a.second;
    if constexpr (PAYLOAD) s.x[w] = a.x;
  }
  __syncthreads();
  Pick<SECOND, PAYLOAD> r;                 // lane k < NW of every wave takes wave k's candidate: one more butterfly
  const int k = threadIdx.x & 63;
  if (k < NW) {
    r.v = s.v[k];
    r.i = s.i[k];
    if constexpr (SECOND) r.second = s.second[k];
    if constexpr (PAYLOAD) r.x = s.x[k];
  }
  return wave_pick(r);
}

// ---- radix selection ---------------------------------------------------------------------------------------------------
// MSB-first radix selection over the order keys of a 1024-thread workgroup (key[j] = 0: absent): returns the largest key `thr`
// such that the total weight of the elements with key > thr is <= T while adding the elements equal to thr would exceed T --
// i.e. "keep key >= thr".  With unit weights and T = k-1 this is the k-th largest value (top-k keeps ties, like `logits < kth`
// removes); with weights = probability mass and T = top_p it is the nucleus boundary (an element is kept iff the mass ranked
// strictly above it is <= top_p, modeling_utils.py:1119-1131).  weight(j) is the integer weight of the thread's element j:
// integer weights make the sums order-independent.
struct RadixLds {
  unsigned long long hist[256];
  unsigned long long acc;
  uint32_t sel;
};
template <int N, typename Weight>
__device__ __forceinline__ uint32_t radix_select(const uint32_t (&key)[N], Weight weight, unsigned long long T, RadixLds& s) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, pmask = 0;
  unsigned long long acc = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) s.hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if ((key[j] & pmask) == prefix && key[j] != 0) {
        const unsigned long long w = weight(j);
        if (w) atomicAdd(&s.hist[(key[j] >> shift) & 255u], w);
      }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long a = acc;
      int d = 255;
      for (; d > 0; --d) {
        if (a + s.hist[d] > T) break;
        a += s.hist[d];
      }
      s.sel = (uint32_t)d;
      s.acc = a;
    }
    __syncthreads();
    prefix |= s.sel << shift;
    pmask |= 255u << shift;
    acc = s.acc;
    __syncthreads();
  }
  return prefix;
}

// ---- per-sequence state of one greedy / sampling step ----------------------------------------------------------------------
// The only copy of the bookkeeping of generate()'s no-beam loop (modeling_utils.py:850-877).  Passed to the step kernels by value.
struct StepState {
  int64_t* ids;          // [B][max_len]
  int32_t* unf;          // [B] 1 while the sequence is unfinished
  float* sum_lp;         // [B] sum of the chosen tokens' log-probs
  float* cnt;            // [B] number of them
  float* logprob_out;    // [B] sum_lp / cnt, written at the last step
  int64_t* raw_last;     // [B] or null: the token chosen at the last step, before the forced [SEP]
  float* margin_out;     // [B][max_len] or null: top-2 margin of the choice
  int32_t* live;         // null or the counter of unfinished sequences (call_state.h)
  int max_len, eos, pad;
  VcEosExtra eos_x;
  // Tokens handed in by the caller (include/vitcap_hip.h: vitcap_greedy_step_forced).  All null / 0 from the plain entry points.
  const int64_t* forced = nullptr;   // [B][max_len] or null: -1 = free, a token id = taken instead of the step's own choice
  float* tok_lp = nullptr;           // [B][max_len] or null: log-prob of the token taken at position t (the caller zeroes the array)
  int score_forced = 0;              // 1: forced tokens enter sum_lp / cnt like chosen ones; 0: they do not (a prompt)

  // the token forced on sequence b at position t, or -1: none (an id outside [0, V) forces nothing)
  __device__ __forceinline__ int forced_at(int b, int t, int V) const {
    if (!forced) return -1;
    const int64_t f = forced[(size_t)b * max_len + t];
    return f >= 0 && f < (int64_t)V ? (int)f : -1;
  }
  // sum_lp / cnt; a sequence none of whose tokens were counted (a prompt that ends it) scores 0
  __device__ __forceinline__ static float mean_lp(float s, float c) { return c > 0.f ? s / c : 0.f; }

  // Finished sequence: tokens_to_add = pad, the score is frozen (modeling_utils.py:855-858, 873-877).  Every thread of the
  // workgroup calls it; true = nothing else to do for sequence b (its logits need not even exist).
  __device__ __forceinline__ bool skip_finished(int b, int t) const {
    if (unf[b] != 0) return false;
    if (threadIdx.x == 0) {
      ids[(size_t)b * max_len + t] = pad;
      if (t == max_len - 1) {
        if (raw_last) raw_last[b] = pad;
        logprob_out[b] = mean_lp(sum_lp[b], cnt[b]);
      }
    }
    return true;
  }
  // Unfinished sequence b takes `token` with log-prob `logprob` at position t; one thread calls it.  Returns what ids[b][t] holds.
  // counted = false: a forced token in prompt mode -- taken like any other, but the score does not see it.
  __device__ __forceinline__ int64_t commit(int b, int t, int token, float logprob, float margin, bool counted = true) const {
    if (margin_out) margin_out[(size_t)b * max_len + t] = margin;
    if (tok_lp) tok_lp[(size_t)b * max_len + t] = logprob;
    const float s = counted ? sum_lp[b] + logprob : sum_lp[b];
    const float c = counted ? cnt[b] + 1.0f : cnt[b];
    const bool open = !vc_is_eos(token, eos, eos_x);   // any id of eos_token_ids finishes the sequence (modeling_utils.py:862-865)
    int64_t outtok = token;
    if (t == max_len - 1) {
      if (raw_last) raw_last[b] = token;               // the token actually chosen, before the forced [SEP]
      if (open) outtok = eos;                          // modeling_utils.py:870-871
      logprob_out[b] = mean_lp(s, c);                  // modeling_utils.py:873-877
    }
    ids[(size_t)b * max_len + t] = outtok;
    sum_lp[b] = s;
    cnt[b] = c;
    unf[b] = open ? 1 : 0;
    if (live && !open) atomicSub(live, 1);
    return outtok;
  }
};
// the state of the call being enqueued: the launcher's arguments plus the engine's per-call thread-locals
static inline StepState vc_step_state(int64_t* ids, int32_t* unf, float* sum_lp, float* cnt, float* logprob_out, int64_t* raw_last,
                                      float* margin_out, int max_len, int eos, int pad, const int64_t* forced = nullptr,
                                      int score_forced = 0, float* tok_lp = nullptr) {
  return StepState{ids, unf, sum_lp, cnt, logprob_out, raw_last, margin_out, (int32_t*)vc_tls_live, max_len, eos, pad, vc_tls_eos_extra,
                   forced, tok_lp, score_forced != 0};
}
