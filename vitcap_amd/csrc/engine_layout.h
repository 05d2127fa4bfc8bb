// Workspace layout of the engine: every buffer is declared ONCE, in VC_WS_BUFFERS below.  Host-only.
#pragma once
#include "../../include/vitcap_hip.h"

namespace vc __attribute__((visibility("hidden"))) {      // nothing of it is exported from the library

constexpr int D = VITCAP_HID;
constexpr int NV = VITCAP_NVIS;        // 577
constexpr int SV = VITCAP_NVIS + 1;    // 578 decoder visual rows (tag CLS first)
constexpr int MASK_WORDS = (SV + 31) / 32;   // 19: uint32 words of one visibility row (vitcap_attn_decode_step_masked)
constexpr int VP = VITCAP_VOCAB_PAD;
constexpr int TOPK = 50;
constexpr int JROWS = 640;           // rows per image of the joint [visual | tag] buffer (578 + 50, padded to 5 x 128)
constexpr int SPLIT_AO = 6, SPLIT_FC2 = 12, SPLIT_MAX = 12;   // split-K of the K=768 / K=3072 decode GEMMs with N=768
constexpr int RS_PIECES = 2 * (VP / 64);                 // 32-column pieces of a logits row ({max, argmax, sum exp, -} each)
constexpr size_t VT_BYTES = (size_t)12 * 64 * 608 * 2;   // one image's transposed visual V rows of one layer (include/vitcap_hip.h: vitcap_attn_beam_vt)

// what a buffer has one unit of: an image (B of them), a decode sequence (NS = B * K of them), or the call
enum Scope { IMG, SEQ, FIXED };

// A placed buffer.  It reads as its byte offset in the workspace (0 and unit == 0: the buffer does not exist in this configuration).
struct Buf {
  size_t off = 0;
  size_t unit = 0;     // bytes per image / per sequence / in all
  Scope scope = FIXED;
  operator size_t() const { return off; }
  // element 0 of unit `i` (image i0 of an IMG buffer, sequence s0 of a SEQ buffer)
  template <class T = char>
  T* at(char* ws, size_t i = 0) const { return (T*)(ws + off + i * unit); }
};

// X(name, scope, bytes per unit, exists) / XA(name, count, ...) for `count` equal buffers in a row (one per decoder layer).
// The ORDER is the order in the workspace.  In the expressions: L = max_length, NT = tag_visible, S = cbs_states, KB = num_beams,
// two = several sequences per image, beam / cbs = the search mode.
// Image-sized buffers come first, so that their offsets do not depend on the number of decode sequences.
#define VC_WS_BUFFERS(X, XA)                                                                                                       \
  X(patches, IMG, 576 * D * 2, true)                                                                                               \
  X(x, IMG, NV * D * 4, true)                                                                                                      \
  X(x2, IMG, NV * D * 4, true)     /* caption branch after the fork (blocks 8-11); x keeps the fork state, read by both */         \
  X(xt, IMG, NV * D * 4, true)                                                                                                     \
  X(h, IMG, SV * D * 2, true)                                                                                                      \
  X(qkv, IMG, NV * 3 * D * 2, true)                                                                                                \
  X(mlp, IMG, SV * 4 * D * 2, true)                                                                                                \
  X(th, IMG, NV * D * 2, true)     /* tag branch's own LN / qkv / MLP temporaries (it runs concurrently) */                        \
  X(tqkv, IMG, NV * 3 * D * 2, true)                                                                                               \
  X(tmlp, IMG, NV * 4 * D * 2, true)                                                                                               \
  X(vis_f, IMG, SV * D * 4, true)                                                                                                  \
  X(vis_b, IMG, SV * D * 2, true)                                                                                                  \
  XA(dqkv, 4, IMG, SV * 3 * D * 2, true)                                                                                           \
  X(da_f, IMG, SV * D * 4, true)                                                                                                   \
  X(da_b, IMG, SV * D * 2, true)                                                                                                   \
  X(dtmp, IMG, SV * D * 4, true)                                                                                                   \
  X(pool_in, IMG, D * 2, true)                                                                                                     \
  X(pooled, IMG, D * 2, true)                                                                                                      \
  X(tg_f, IMG, D * 4, true)                                                                                                        \
  X(tg_b, IMG, D * 2, true)                                                                                                        \
  X(tag_logits, IMG, VP * 4, true)                                                                                                 \
  X(tag_ids, IMG, TOPK * 8, true)                                                                                                  \
  X(tag_prob, IMG, TOPK * 4, true)                                                                                                 \
  X(tag_len, IMG, 8, true)                                                                                                         \
  /* step buffers: two rows (token t-1, [MASK]) per sequence */                                                                    \
  X(xs_f, SEQ, 2 * D * 4, true)                                                                                                    \
  X(xs_b, SEQ, 2 * D * 2, true)                                                                                                    \
  X(sqkv, SEQ, 2 * 3 * D * 2, true)                                                                                                \
  X(sctx, SEQ, 2 * D * 2, true)                                                                                                    \
  X(spart, SEQ, SPLIT_MAX * 2 * D * 4, true)   /* split-K partial slabs of the decode-step GEMMs */                                \
  X(sa_f, SEQ, 2 * D * 4, true)                                                                                                    \
  X(sa_b, SEQ, 2 * D * 2, true)                                                                                                    \
  X(smlp, SEQ, 2 * 4 * D * 2, true)                                                                                                \
  X(tcache, SEQ, 4 * L * 2 * D * 2, true)      /* text K/V history, LAYER-major: see tcache_at() */                                \
  X(tcache2, SEQ, 4 * L * 2 * D * 2, two)                                                                                          \
  X(hd_f, SEQ, D * 4, true)                                                                                                        \
  X(hd_b, SEQ, D * 2, true)                                                                                                        \
  X(logits, SEQ, VP * 4, true)                                                                                                     \
  X(rowstat, SEQ, RS_PIECES * 16, true)                                                                                            \
  X(ids, SEQ, L * 8, true)                                                                                                         \
  X(ids2, SEQ, L * 8, two)                                                                                                         \
  X(unf, SEQ, 4, true)                                                                                                             \
  X(sum_lp, SEQ, 4, true)                                                                                                          \
  X(cnt, SEQ, 4, true)                                                                                                             \
  X(margins, SEQ, L * 4, true)                                                                                                     \
  X(logprob, SEQ, 4, true)                                                                                                         \
  X(last_tok, SEQ, 8, true)                                                                                                        \
  /* forced decoding (vitcap_engine_decode_forced): the call's copy of the caller's tokens and the per-token log-probs */         \
  X(forced, SEQ, L * 8, !beam && !cbs)                                                                                             \
  X(tok_lp, SEQ, L * 4, !beam && !cbs)                                                                                             \
  X(live, FIXED, 256, true)                                                                                                        \
  /* tag rows visible to the caption (tag_visible = NT > 0), per embedding branch A / B: state, then per decoder layer the tag */  \
  /* rows' packed q|k|v = their K/V cache */                                                                                       \
  X(tagx_f_a, IMG, NT * D * 4, NT > 0)                                                                                             \
  X(tagx_b_a, IMG, NT * D * 2, NT > 0)                                                                                             \
  XA(tqkv_c_a, 4, IMG, NT * 3 * D * 2, NT > 0)                                                                                     \
  X(tagx_f_b, IMG, NT * D * 4, NT > 0)                                                                                             \
  X(tagx_b_b, IMG, NT * D * 2, NT > 0)                                                                                             \
  XA(tqkv_c_b, 4, IMG, NT * 3 * D * 2, NT > 0)                                                                                     \
  X(jqkv, IMG, JROWS * 3 * D * 2, NT > 0)      /* per image [578 visual K/V | n tag rows] for the tag rows' attention */           \
  X(jout, IMG, JROWS * D * 2, NT > 0)                                                                                              \
  X(jlse, IMG, 12 * JROWS * 4, NT > 0)                                                                                             \
  X(tg_ctx, IMG, NT * D * 2, NT > 0)                                                                                               \
  X(tg_sa_f, IMG, NT * D * 4, NT > 0)                                                                                              \
  X(tg_sa_b, IMG, NT * D * 2, NT > 0)                                                                                              \
  X(tg_mlp, IMG, NT * 4 * D * 2, NT > 0)                                                                                           \
  X(tg_tmp, IMG, NT * D * 4, NT > 0)                                                                                               \
  /* per decoder layer the visual V rows transposed per (image, head) for vitcap_attn_decode_beams */                              \
  XA(vt, 4, IMG, VT_BYTES, (beam || cbs) && NT == 0)                                                                               \
  /* constrained beam search: S * KB candidates per sequence (KB words for each of the S target states) */                         \
  X(cbs_val, SEQ, S * KB * 4, cbs)                                                                                                 \
  X(cbs_word, SEQ, S * KB * 4, cbs)                                                                                                \
  X(cbs_sc, SEQ, 4, cbs)                                                                                                           \
  X(cbs_sc2, SEQ, 4, cbs)                                                                                                          \
  X(cbs_unf, FIXED, L * 4, cbs)                                                                                                    \
  X(cbs_npred, FIXED, 256, cbs)                                                                                                    \
  X(cbs_flags, IMG, S * S, cbs)                                                                                                    \
  X(cbs_lse, SEQ, 4, cbs)                                                                                                          \
  X(cbs_max, SEQ, 4, cbs)          /* row maxima next to the log-sum-exp (vitcap_row_topk_lse with k = 1) */                       \
  X(cbs_argmax, SEQ, 4, cbs)                                                                                                       \
  X(cbs_parent, SEQ, 4, cbs)                                                                                                       \
  X(cbs_fin_ids, IMG, L * 8, cbs)                                                                                                  \
  X(cbs_fin_lp, IMG, 4, cbs)                                                                                                       \
  /* beam search: 2 * beams <= 16 candidates per sequence; up to 8 kept hypotheses per image (num_keep_best) */                    \
  X(cand_val, SEQ, 16 * 4, beam)                                                                                                   \
  X(cand_idx, SEQ, 16 * 4, beam)                                                                                                   \
  X(lse, SEQ, 4, beam)                                                                                                             \
  X(beam_scores, SEQ, 4, beam)                                                                                                     \
  X(parent, SEQ, 4, beam)                                                                                                          \
  X(done, IMG, 4, beam)                                                                                                            \
  X(has_hyp, IMG, 4, beam)                                                                                                         \
  X(hyp_score, IMG, 8 * 4, beam)                                                                                                   \
  X(hyp_len, IMG, 8 * 4, beam)                                                                                                     \
  X(hyp_tok, IMG, 8 * L * 8, beam)                                                                                                 \
  X(fin_ids, IMG, 8 * L * 8, beam)                                                                                                 \
  X(fin_lp, IMG, 8 * 4, beam)

struct Layout {
#define VC_DECL(name, ...) Buf name;
#define VC_DECL_A(name, count, ...) Buf name[count];
  VC_WS_BUFFERS(VC_DECL, VC_DECL_A)
#undef VC_DECL
#undef VC_DECL_A
  size_t off = 0;    // bytes taken so far; after the constructor: the workspace size
  int NT = 0;        // tag rows per image visible to the caption
  int L = 0, NS = 0, K = 0;
  int group_k = 1;   // K > 8: the largest divisor of K that is <= 8 (sequences per attention workgroup), 1 if K is a prime above 8
  bool beam = false;
  bool cbs = false;  // constrained beam search: K = cbs_states * num_beams sequences per image

  Layout() {}
  Layout(int B, const vitcap_gen_opts& o) {
    L = o.max_length;
    NT = o.tag_visible;
    cbs = o.use_cbs != 0;
    beam = !cbs && o.num_beams > 1;
    K = cbs ? o.cbs_states * o.num_beams : (beam ? o.num_beams : o.seqs_per_image);
    NS = B * K;
    for (int g = 8; g >= 2; --g)
      if (K % g == 0) { group_k = g; break; }
    const bool two = K > 1 || cbs;                // layouts with several sequences per image carry the second cache / id buffer
    const size_t S = (size_t)o.cbs_states, KB = (size_t)o.num_beams;
    const size_t units[3] = {(size_t)B, (size_t)NS, 1};
    auto place = [&](Buf* b, int count, Scope sc, size_t unit, bool exists) {
      for (int i = 0; i < count && exists; ++i) {
        b[i] = Buf{off, unit, sc};
        off += (units[sc] * unit + 255) & ~(size_t)255;
      }
    };
#define VC_PLACE(name, scope, bytes, exists) place(&name, 1, scope, (size_t)(bytes), exists);
#define VC_PLACE_A(name, count, scope, bytes, exists) place(name, count, scope, (size_t)(bytes), exists);
    VC_WS_BUFFERS(VC_PLACE, VC_PLACE_A)
#undef VC_PLACE
#undef VC_PLACE_A
  }

  // the same layout seen from image i0 on: every per-image buffer advanced by i0 images
  Layout from_image(int i0) const {
    Layout v = *this;
    auto shift = [&](Buf* b, int count) {
      for (int i = 0; i < count; ++i)
        if (b[i].scope == IMG) b[i].off += (size_t)i0 * b[i].unit;
    };
#define VC_SHIFT(name, ...) shift(&v.name, 1);
#define VC_SHIFT_A(name, count, ...) shift(v.name, count);
    VC_WS_BUFFERS(VC_SHIFT, VC_SHIFT_A)
#undef VC_SHIFT
#undef VC_SHIFT_A
    return v;
  }

  // tag rows visible to the caption, embedding branch v in {A, B}
  const Buf& tagx_f(int v) const { return v ? tagx_f_b : tagx_f_a; }
  const Buf& tagx_b(int v) const { return v ? tagx_b_b : tagx_b_a; }
  const Buf& tqkv_c(int v, int l) const { return v ? tqkv_c_b[l] : tqkv_c_a[l]; }
  // byte offset, inside a text K/V cache [4 layers][NS][L][2][D] bf16, of the history of sequence s0 in layer l
  size_t tcache_at(int l, size_t s0) const { return ((size_t)l * NS + s0) * L * 2 * D * 2; }
};

// ---- the score workspace of the one-pass caption scorer (vitcap_engine_score*) ---------------------------------------------------
// A second caller-provided block, separate from the table above (whose rows and sizes it leaves alone).  Units: NC = B * K
// captions, M = NC * (2L - 1) grid rows, P = NC * (L - 1) probe rows, CH = min(P, SCORE_CHUNK) rows of one vocabulary-GEMM chunk.
// Sizes at L = 20: 64 images x 5 captions 0.66 GB, 64 x 32 captions 2.51 GB, of which the logits chunk is 0.25 GB (unchunked it
// would be 4.7 GB at 64 x 32).
constexpr int SCORE_CHUNK = 2048;      // probe rows per vocabulary GEMM: the large-tile forms are at full size from 2048 rows on
constexpr int SCORE_MAX_CAPS = 32;     // captions per image

#define VC_SCORE_BUFFERS(X)                                                                                                        \
  X(ids, NC, L * 8)              /* the call's copy of the caller's captions */                                                    \
  X(last_tok, NC, 8)             /* ... and of last_tok (-1 everywhere when none is given) */                                      \
  X(grid_ids, M, 8)              /* [tokens | [MASK] x (L-1)] per caption, for vitcap_embed_rows */                                \
  X(x_f, M, D * 4)               /* residual stream */                                                                             \
  X(x_b, M, D * 2)                                                                                                                 \
  X(qkv, M, 3 * D * 2)                                                                                                             \
  X(ctx, M, D * 2)                                                                                                                 \
  X(tmp, M, D * 4)               /* GEMM output in front of a LayerNorm */                                                         \
  X(sa_f, M, D * 4)                                                                                                                \
  X(sa_b, M, D * 2)                                                                                                                \
  X(mlp, M, 4 * D * 2)                                                                                                             \
  X(vt, B, VT_BYTES)             /* V^T of the current layer's visual rows (vitcap_attn_beam_vt), rewritten per layer */           \
  X(hd_in, P, D * 2)             /* the probe rows of the last layer, compact */                                                   \
  X(hd_f, P, D * 4)                                                                                                                \
  X(hd_b, P, D * 2)                                                                                                                \
  X(logits, CH, VP * 4)                                                                                                            \
  X(tok_lp, NC, L * 4)           /* per-token log-probs when the caller wants none */

struct ScoreLayout {
#define VC_DECL(name, ...) Buf name;
  VC_SCORE_BUFFERS(VC_DECL)
#undef VC_DECL
  size_t off = 0;
  int B = 0, K = 0, L = 0, R = 0;
  size_t NC = 0, M = 0, P = 0, CH = 0;

  ScoreLayout() {}
  ScoreLayout(int B_, int K_, int L_) : B(B_), K(K_), L(L_), R(2 * L_ - 1) {
    NC = (size_t)B * K;
    M = NC * R;
    P = NC * (L - 1);
    CH = P < (size_t)SCORE_CHUNK ? P : (size_t)SCORE_CHUNK;
#define VC_PLACE(name, count, bytes)                                \
  name = Buf{off, (size_t)(bytes), FIXED};                          \
  off += ((size_t)(count) * (size_t)(bytes) + 255) & ~(size_t)255;
    VC_SCORE_BUFFERS(VC_PLACE)
#undef VC_PLACE
  }
};

}  // namespace vc
