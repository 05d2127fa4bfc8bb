// One probe row of the one-pass caption scorer, stated once: which rows are live, which token a row scores, the log-prob expression
// and what the row writes.  Used by score_rows_kernel (decode.hip) and by the alternatives kernel (alternatives.hip), which does the
// same job from the registers it already holds: both give the same bits because both go through these functions and keep one
// summation order (thread-strided partial sums of score_row_term, element tid + j * 1024 in round j, then block_sum<16>).
#pragma once
#include "common.h"
#include "select.h"

struct ScoreArgs {
  const int64_t* ids;        // [n_caps][L] the captions
  const int64_t* last_tok;   // [n_caps] or null
  float* tok_lp;             // [n_caps][L]
  int64_t* out_ids;          // [n_caps][L]
  int64_t* out_last;         // [n_caps] or null
  float *sum_lp, *cnt, *logprob;      // [n_caps] (sum_lp / cnt may be null)
  int L, eos, pad;
  VcEosExtra eos_x;
};

// decode.hip: score_finish_kernel, the sums of the captions whose last probe row lies in [rows0, rows0 + n_rows)
int vc_score_finish(const ScoreArgs& a, int n_caps, int rows0, int n_rows, void* stream);

// probe row g of the grid = caption g / (L-1), position t = g % (L-1) + 1
__device__ __forceinline__ void score_row_place(int g, int L, int& b, int& t) {
  b = g / (L - 1);
  t = g - b * (L - 1) + 1;
}
// an EOS id strictly before position t: the row lies behind its caption's end
__device__ __forceinline__ bool score_row_ended(const int64_t* cap, int t, int eos, const VcEosExtra& eos_x) {
  bool ended = false;
  for (int j = 1; j < t; ++j) ended = ended || vc_is_eos((int)cap[j], eos, eos_x);
  return ended;
}
// The token a live row scores: the given one when it is an id of the vocabulary, else the row's argmax; in the last column a written
// [SEP] is the max-length rule's, not a choice: the caller's token, or the row's argmax.
__device__ __forceinline__ int score_row_token(const int64_t* cap, const int64_t* last_tok, int b, int t, int L, int eos, int V, int argmax) {
  const int64_t given = cap[t];
  int f = given >= 0 && given < (int64_t)V ? (int)given : argmax;
  if (t == L - 1 && given == (int64_t)eos) {
    const int64_t lt = last_tok ? last_tok[b] : -1;
    f = lt >= 0 && lt < (int64_t)V ? (int)lt : argmax;
  }
  return f;
}
// one element's term of S = sum exp(x - m), and the log-prob of an element given m = max x and S
__device__ __forceinline__ float score_row_term(float x, float m) { return expf(x - m); }
__device__ __forceinline__ float score_row_lp(float x, float m, float S) { return (x - m) - logf(S); }

// what a row behind the end writes (the stepwise loop's skip_finished); one thread calls it
__device__ __forceinline__ void score_row_write_dead(const ScoreArgs& a, int b, int t) {
  const size_t o = (size_t)b * a.L + t;
  a.tok_lp[o] = 0.f;
  a.out_ids[o] = a.pad;
  if (t == a.L - 1 && a.out_last) a.out_last[b] = a.pad;
}
// what a live row writes for its scored token f; one thread calls it
__device__ __forceinline__ void score_row_write(const ScoreArgs& a, int b, int t, int f, float lp) {
  const size_t o = (size_t)b * a.L + t;
  a.tok_lp[o] = lp;
  int64_t outtok = f;
  if (t == a.L - 1) {
    if (a.out_last) a.out_last[b] = f;
    if (!vc_is_eos(f, a.eos, a.eos_x)) outtok = a.eos;      // modeling_utils.py:870-871
  }
  a.out_ids[o] = outtok;
}
