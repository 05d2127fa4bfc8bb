// Engine: enqueues the whole greedy-captioning forward of ViTCAP on one HIP stream.
//
//   encode  : patch embed -> 8 shared ViT blocks -> fork -> 4 caption blocks + 4 tag blocks   (a1-a5)
//             tag head (pooler, transform, 30522-way classifier, sigmoid top-50)                (a6)
//   prefill : [tag CLS | 577 visual] rows through the 4 post-LN decoder layers ONCE; the per-layer packed
//             qkv buffers stay resident as the visual K/V cache                                  (a8/a9)
//   decode  : 19 steps x (2 query rows per sequence through 4 layers against the caches, LM head on the
//             [MASK] row, device-side greedy bookkeeping) -- no host synchronisation             (a9-a12)
//
// The reference recomputes encode+prefill at every step (modeling_utils.py:798-867 with past=None,
// SURVEY.md headline 4); the result is the same because visual rows never attend text rows under the
// seq2seq mask (..._bertemb.py:57-85) and text rows attend only earlier text rows (dataset.py:377-390).
// The 50 tag slots of the text segment are attended by nothing and their outputs are discarded
// (SURVEY.md headline 5), so they are not materialised; the tag head itself is still computed and exposed.
#include <stdlib.h>
#include <string.h>

#include <new>
#include <utility>

#include "engine_internal.h"
#include "engine_layout.h"

using namespace vc;

namespace {

vitcap_gen_opts default_opts() {
  vitcap_gen_opts o;
  memset(&o, 0, sizeof(o));
  o.abi = VITCAP_ABI_VERSION;
  o.num_beams = 1;
  o.seqs_per_image = 1;
  o.num_keep_best = 1;
  o.max_length = VITCAP_MAXLEN;
  o.bos_token_id = 101; o.eos_token_id = 102; o.pad_token_id = 0; o.mask_token_id = 103;
  o.length_penalty = 1.0f;
  o.repetition_penalty = 1.0f;
  o.sampling.do_sample = 0; o.sampling.temperature = 1.0f; o.sampling.top_k = 0; o.sampling.top_p = 1.0f; o.sampling.seed = 0u;
  o.gemm_mode = VITCAP_GEMM_AUTO;
  o.early_exit = 1;
  o.use_graph = 0;
  o.tag_visible = 0;
  o.tagemb_cls = 1;
  o.decode_streams = 0;
  o.encode_parts = 0;
  o.eos_extra[0] = o.eos_extra[1] = o.eos_extra[2] = -1;
  o.tag_pos0 = VITCAP_MAXLEN;
  o.use_cbs = 0; o.cbs_states = 0; o.min_constraints_to_satisfy = 2; o.cbs_no_repeat = 0;
  for (int i = 0; i < 16; ++i) o.cbs_bad_ending[i] = -1;
  o.fsm = nullptr; o.num_constraints = nullptr;
  return o;
}

int check_opts(const vitcap_gen_opts& o) {
#define OPT_REQ(cond, ...) do { if (!(cond)) { vitcap_set_error(__VA_ARGS__); return VITCAP_EINVAL; } } while (0)
  OPT_REQ(o.abi == VITCAP_ABI_VERSION, "gen_opts: built against ABI %d, this library is ABI %d (use vitcap_gen_opts_init)", o.abi, VITCAP_ABI_VERSION);
  OPT_REQ(o.num_beams >= 1 && o.num_beams <= 8, "gen_opts: num_beams must be 1..8 (got %d)", o.num_beams);
  OPT_REQ(o.seqs_per_image >= 1 && o.seqs_per_image <= 8, "gen_opts: seqs_per_image must be 1..8 (got %d)", o.seqs_per_image);
  OPT_REQ(o.num_keep_best >= 1 && o.num_keep_best <= 8, "gen_opts: num_keep_best must be 1..8 (got %d)", o.num_keep_best);
  OPT_REQ(!(o.num_beams > 1 && o.seqs_per_image > 1), "gen_opts: seqs_per_image > 1 needs num_beams == 1");
  OPT_REQ(!(o.num_beams == 1 && o.num_keep_best > 1), "gen_opts: cannot generate >1 sentences in greedy search (num_keep_best > 1 needs num_beams > 1)");
  OPT_REQ(o.max_length >= 2 && o.max_length <= VITCAP_MAXLEN_CAP, "gen_opts: max_length must be 2..%d (got %d)", VITCAP_MAXLEN_CAP, o.max_length);
  const int32_t toks[4] = {o.bos_token_id, o.eos_token_id, o.pad_token_id, o.mask_token_id};
  for (int i = 0; i < 4; ++i) OPT_REQ(toks[i] >= 0 && toks[i] < VITCAP_VOCAB, "gen_opts: token id %d out of the vocabulary", toks[i]);
  OPT_REQ(o.repetition_penalty > 0.f, "gen_opts: repetition_penalty must be > 0 (got %g)", (double)o.repetition_penalty);
  OPT_REQ(!o.sampling.do_sample || (o.sampling.temperature > 0.f && o.sampling.top_k >= 0 && o.sampling.top_p > 0.f),
          "gen_opts: temperature %g / top_k %d / top_p %g out of range", (double)o.sampling.temperature, o.sampling.top_k, (double)o.sampling.top_p);
  OPT_REQ(o.gemm_mode == VITCAP_GEMM_AUTO || o.gemm_mode == VITCAP_GEMM_TILES, "gen_opts: gemm_mode %d unknown", o.gemm_mode);
  OPT_REQ(o.tag_visible >= 0 && o.tag_visible <= 50, "gen_opts: tag_visible must be 0..50 (got %d)", o.tag_visible);
  OPT_REQ(o.tag_pos0 >= VITCAP_MAXLEN && o.tag_pos0 <= 512 - 50, "gen_opts: tag_pos0 must be %d..462 (got %d)", VITCAP_MAXLEN, o.tag_pos0);
  OPT_REQ(o.tag_visible == 0 || o.max_length == VITCAP_MAXLEN, "gen_opts: tag_visible > 0 needs max_length == %d", VITCAP_MAXLEN);
  OPT_REQ(o.encode_parts >= 0 && o.encode_parts <= 4, "gen_opts: encode_parts must be 0 (auto) .. 4 (got %d)", o.encode_parts);
  OPT_REQ(o.decode_streams >= 0 && o.decode_streams <= 2, "gen_opts: decode_streams must be 0 (auto), 1 or 2 (got %d)", o.decode_streams);
  for (int i = 0; i < 3; ++i) {
    OPT_REQ(o.eos_extra[i] >= -1 && o.eos_extra[i] < VITCAP_VOCAB, "gen_opts: eos_extra[%d] = %d is neither -1 nor a token id", i, o.eos_extra[i]);
    // the reference's own beam search does not survive several EOS ids: more than num_beams of the 2*num_beams candidates can then
    // be EOS words and `assert len(next_sent_beam) == num_beams` fires (modeling_utils.py:1037)
    OPT_REQ(o.eos_extra[i] < 0 || o.num_beams == 1, "gen_opts: several eos_token_ids need num_beams == 1 (the reference's beam search asserts with them)");
  }
  if (o.use_cbs) {
    // ViTCAP.generate(use_cbs=True): utils_cbs.py keeps num_keep_best = 1 and a plain log-softmax (modeling_bert.py:1038-1042)
    OPT_REQ(o.use_cbs == 1, "gen_opts: use_cbs must be 0 or 1 (got %d)", o.use_cbs);
    OPT_REQ(o.fsm && o.num_constraints, "gen_opts: use_cbs needs fsm [B][S][S][%d] uint8 and num_constraints [B] int64 on the device "
            "(the reference reads fsm.shape, modeling_bert.py:952)", VITCAP_VOCAB);
    OPT_REQ(o.cbs_states >= 1 && o.cbs_states <= 32, "gen_opts: cbs_states must be 1..32 (got %d)", o.cbs_states);
    OPT_REQ(o.cbs_states * o.num_beams <= 256, "gen_opts: cbs_states * num_beams must be <= 256 sequences per image (got %d)",
            o.cbs_states * o.num_beams);
    OPT_REQ(o.min_constraints_to_satisfy >= 0, "gen_opts: min_constraints_to_satisfy must be >= 0 (got %d)", o.min_constraints_to_satisfy);
    OPT_REQ(o.num_keep_best == 1, "gen_opts: not supported n_best > 1 for CBS (modeling_bert.py:1038)");
    OPT_REQ(o.seqs_per_image == 1 && !o.sampling.do_sample && o.repetition_penalty == 1.0f,
            "gen_opts: use_cbs runs neither sampling, num_return_sequences > 1 nor the repetition penalty (utils_cbs.py:184-185)");
    OPT_REQ(o.tag_visible == 0, "gen_opts: use_cbs with tag tokens visible to the caption is not built");
    OPT_REQ(o.max_length >= 3, "gen_opts: use_cbs needs max_length >= 3 (got %d)", o.max_length);
    OPT_REQ(o.cbs_no_repeat == 0 || o.cbs_no_repeat == 1, "gen_opts: cbs_no_repeat must be 0 or 1 (got %d)", o.cbs_no_repeat);
    for (int i = 0; i < 16; ++i)
      OPT_REQ(o.cbs_bad_ending[i] >= -1 && o.cbs_bad_ending[i] < VITCAP_VOCAB, "gen_opts: cbs_bad_ending[%d] = %d is neither -1 nor a token id", i, o.cbs_bad_ending[i]);
  }
#undef OPT_REQ
  return VITCAP_OK;
}

#define CK(call)             \
  do {                       \
    int rc_ = (call);        \
    if (rc_ != 0) return rc_; \
  } while (0)

#define HIPCK(call, what)                                                              \
  do {                                                                                 \
    hipError_t he_ = (call);                                                           \
    if (he_ != hipSuccess) {                                                           \
      vitcap_set_error("%s: %s", what, hipGetErrorString(he_));                        \
      return VITCAP_ELAUNCH;                                                           \
    }                                                                                  \
  } while (0)

void drop_graphs(vitcap_engine* e) {
  for (auto& g : e->graphs) {
    (void)hipGraphExecDestroy(g.exec);
    (void)hipGraphDestroy(g.graph);
  }
  e->graphs.clear();
}

// The engine's helper streams are PROCESS-wide, one per role and device, created on first use and never destroyed.  HIP maps streams onto a
// few hardware queues (GPU_MAX_HW_QUEUES, default 4) in creation order, and two chains that share a queue block each other at every
// event wait.  With streams owned by the engine object, every new model of a process (pipeline_eval_multi over several test sets) drew a
// new arrangement: some put the encoder and the decode chain on one queue and the 2-slot pipeline ran at HALF its rate (measured: the
// second and third predict() of a process 1 935 instead of 3 750 images/s, all fine with 8 queues; profiles/r05_hw_queue_aliasing.txt).
// Shared streams add ordering between two engines used at the same time from two threads, never a hazard: every use is fenced by the
// engine's own events.
enum { ROLE_SIDE = 0, ROLE_DEC2 = 1, ROLE_PART0 = 2 /* .. +2 */, ROLE_COUNT = 5 };
hipStream_t role_stream(int role) {
  static std::mutex mu;
  static hipStream_t pool[64][ROLE_COUNT] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || role < 0 || role >= ROLE_COUNT) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!pool[dev][role] && hipStreamCreateWithFlags(&pool[dev][role], hipStreamNonBlocking) != hipSuccess) pool[dev][role] = nullptr;
  return pool[dev][role];
}

// First use of a helper stream by this engine: the role's stream and whichever of its fork / join events do not exist yet.
int ensure_lane(int role, hipStream_t& st, hipEvent_t& ev_fork, hipEvent_t& ev_join, const char* what) {
  if (st) return VITCAP_OK;
  hipStream_t rs = role_stream(role);
  if (!rs || (!ev_fork && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) ||
      (!ev_join && hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess)) {
    vitcap_set_error("%s stream creation failed", what);
    return VITCAP_ELAUNCH;
  }
  st = rs;
  return VITCAP_OK;
}
int ev_record(hipEvent_t ev, void* s, const char* what, const char* edge) {
  const hipError_t he = hipEventRecord(ev, (hipStream_t)s);
  if (he != hipSuccess) { vitcap_set_error("%s %s record: %s", what, edge, hipGetErrorString(he)); return VITCAP_ELAUNCH; }
  return VITCAP_OK;
}
int ev_wait(void* s, hipEvent_t ev, const char* what, const char* edge) {
  const hipError_t he = hipStreamWaitEvent((hipStream_t)s, ev, 0);
  if (he != hipSuccess) { vitcap_set_error("%s %s wait: %s", what, edge, hipGetErrorString(he)); return VITCAP_ELAUNCH; }
  return VITCAP_OK;
}
// `to` goes on behind everything enqueued on `from` so far: a chain starts on `to` (fork) or hands its work back to `to` (join)
int fork(void* from, void* to, hipEvent_t ev, const char* what) {
  CK(ev_record(ev, from, what, "fork"));
  return ev_wait(to, ev, what, "fork");
}
int join(void* from, void* to, hipEvent_t ev, const char* what) {
  CK(ev_record(ev, from, what, "join"));
  return ev_wait(to, ev, what, "join");
}

vitcap_gemm_desc desc(int M, int N, int K, int lda, int ldc, int act, int out) {
  vitcap_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.abi = VITCAP_ABI_VERSION;
  d.M = M; d.N = N; d.K = K;
  d.lda = lda; d.ldw = K; d.ldc = ldc;
  d.act = act; d.out_dtype = out;
  return d;
}

// A contiguous slice of the decode batch: sequences [s0, s0 + ns) = images [i0, i0 + ns / K).  The greedy loop can be cut into
// two such slices that run on two streams (vitcap_gen_opts.decode_streams = 2).  Every decode-step kernel costs ~4.5 us of
// dispatch-to-drain latency whatever its size (31 of them per step: 140 us of a 295 us step at 64 sequences); the experiment
// showed that a second chain does NOT hide it (see greedy_loop).  Results are bit-identical to the unsplit loop.
struct Part {
  int s0, ns, i0;
};

// The context of one enqueueing call: what every launch of the call needs to know, and -- for its lifetime -- the per-call state the
// public launchers read from thread-locals (call_state.h).  ENCODE (encoder and prefill): the streaming kernels zig-zag; DECODE: the
// step kernels carry the early-exit counter.  Nothing leaks out of an engine call: the destructor restores the defaults.
struct Enq {
  enum Phase { ENCODE, DECODE };
  vitcap_engine* const e;
  const vitcap_weights& w;
  const vitcap_gen_opts& o;
  const Layout& lo;          // of the images this context covers (an encoder part: Layout::from_image)
  char* const ws;
  const int B;               // images this context covers
  void* const s;             // stream its launches go to
  const int32_t* const live; // live counter handed to the decode-step launches (null: encoder / prefill, or early_exit off)
  const bool owner;
  // forced decoding (vitcap_engine_decode_forced): -1 = a plain call; 0 / 1 = score_forced, and the greedy loop reads lo.forced
  // (staged by the caller of decode_loop) and writes lo.tok_lp
  int forced = -1;
  // region captions (vitcap_engine_decode_masked): the caller's device array [NS][MASK_WORDS], read in place by the attention launches
  const uint32_t* vis_mask = nullptr;
  // patch removal (vitcap_engine_encode_patches / _prefill_patches): the caller's device array [B][MASK_WORDS] in cache order, row 0 =
  // the first image THIS context covers; every dense attention launch of the encoder (bit0 = 1) and of the prefill (bit0 = 0) reads it
  const uint32_t* patch_mask = nullptr;
  // encoder attention written out (vitcap_engine_encode_maps): the selection and the caller's device array; null = a plain call
  struct BlockMaps {
    float* out;              // [n_sel][B][H'][NV][NV], the selected blocks in ascending bit order
    uint32_t mask;           // bits 0..11 blocks[0..11], 12..15 tag_blocks[0..3]
    int per_head;
  };
  const BlockMaps* block_maps = nullptr;

  Enq(vitcap_engine* e, int B, const vitcap_gen_opts& o, const Layout& lo, char* ws, void* s, Phase ph)
      : e(e), w(e->w), o(o), lo(lo), ws(ws), B(B), s(s),
        live(ph == DECODE && o.early_exit ? lo.live.at<int32_t>(ws) : nullptr), owner(true) {
    vc_tls_live = live;
    vc_tls_eos_extra = VcEosExtra{{o.eos_extra[0], o.eos_extra[1], o.eos_extra[2]}};
    vc_tls_walk_rev = false;
    vc_tls_zigzag = ph == ENCODE;
  }
  ~Enq() {
    if (!owner) return;
    vc_tls_live = nullptr;
    vc_tls_eos_extra = VcEosExtra{{-1, -1, -1}};
    vc_tls_walk_rev = vc_tls_zigzag = false;
  }
  Enq(const Enq&) = delete;
  // the same call seen by another chain of it: other images and / or another stream
  // first_image: the view's first image within this context (a part reads its own images' rows of patch_mask)
  Enq view(const Layout& lv, int Bv, void* sv, int first_image = 0) const { return Enq(*this, lv, Bv, sv, first_image); }
  Enq on(void* sv) const { return view(lo, B, sv); }

  template <class T = char>
  T* p(const Buf& b, size_t i = 0) const { return b.at<T>(ws, i); }

  // Zig-zag walk of the encoder / prefill chain (call_state.h: vc_tls_walk_rev): `zz()` after every streaming launch flips the
  // direction for the next one, so that each kernel starts on the rows its producer wrote last (still in the Infinity Cache).
  static void zz() { vc_tls_walk_rev = !vc_tls_walk_rev; }

  int gemm_desc(const void* A, const void* W, const float* bias, const float* res, void* C, vitcap_gemm_desc d) const {
    // the big-tile launches of the encoder / prefill (the decode-step GEMMs of large batches are a different, latency-bound population)
    bool eligible = e->timing && d.M >= 2048;
    if (eligible) {      // a launch that is being captured into a hipGraph cannot carry events that are queried afterwards
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing((hipStream_t)s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) eligible = false;
    }
    const bool timed = eligible && e->timing_this_step && e->used < e->pool.size();
    GemmTiming* t = timed ? &e->pool[e->used++] : nullptr;
    // one tile per workgroup for the large GEMMs when the caller overlaps a second stream (vitcap_gen_opts.gemm_mode)
    if (d.tile_hint == 0 && o.gemm_mode == VITCAP_GEMM_TILES && d.M >= 2048 && d.act != VITCAP_ACT_TANH && d.split_k <= 1) {
      d.tile_hint = 5;
      // Round 6: from 64k rows per launch on (B = 512) the bf16-output GEMMs (qkv, fc1) run the PERSISTENT 4-wave form, whose A-panel
      // prefetch exists for that size class (gemm4w.hip PF) -- +0.4-0.9 % images/s, -1 % joules per step at B = 512
      // (profiles/r06_prefetch_ab_b512.txt) -- but only next to a greedy decode chain (the other stream's chain is a plain greedy /
      // sampling loop of <= 512 sequences): beside the 1 280-sequence chain of beam 5 x 256 the persistent grids cost -3.4 %
      // (3 688 -> 3 562 img/s, profiles/r06_decode_forms_and_beam_ab.txt).
      const bool light_decode = o.num_beams <= 1 && o.cbs_states <= 1;
      if (light_decode && d.M >= 65536 && d.out_dtype == VITCAP_OUT_BF16 && !res && (d.N & 255) == 0 && d.K >= 192 && d.row_group == 0 &&
          !d.colsum && !d.rowstat)
        d.tile_hint = 42;
    }
    if (d.M <= 4096) d.live = live;           // decode-step shapes only; the encoder / prefill GEMMs never carry it
    if (t) {
      t->variant = d.act * 4 + d.out_dtype * 2 + (res ? 1 : 0);
      t->flops = 2.0 * d.M * d.N * d.K;
      (void)hipEventRecord(t->start, (hipStream_t)s);
      vc_tls_kev_start = t->kstart;
      vc_tls_kev_stop = t->kstop;
      vc_tls_kev_used = false;
    }
    const int rc = vitcap_gemm_bias_act(A, W, bias, res, C, &d, s);
    if (t) {
      t->kernel_bound = vc_tls_kev_used;
      vc_tls_kev_start = vc_tls_kev_stop = nullptr;
      (void)hipEventRecord(t->stop, (hipStream_t)s);
    }
    return rc;
  }

  int gemm(const void* A, int lda, const void* W, const float* bias, const float* res, int ldr, void* C, int ldc, int M, int N, int K,
           int act, int out) const {
    vitcap_gemm_desc d = desc(M, N, K, lda, ldc, act, out);
    d.ldr = ldr;
    return gemm_desc(A, W, bias, res, C, d);
  }

  // residual GEMM (N = 768, fp32 out) + LayerNorm of its finished rows -> ln_b (bf16) / ln_f (fp32, optional).  No ln_counters are handed
  // over, so vitcap_gemm_ex launches the LayerNorm kernel behind the GEMM: the in-kernel LayerNorm is bit-identical and SLOWER
  // (docs/LAB_r01_r04.md 4.3)
  int gemm_ln(const void* A, int lda, const void* W, const float* bias, const float* res, void* C, int M, int K, const float* g,
              const float* beta, float eps, void* ln_b, float* ln_f) const {
    vitcap_gemm_desc d = desc(M, D, K, lda, D, VITCAP_ACT_NONE, VITCAP_OUT_F32);
    d.ldr = D;
    d.ln_gamma = g; d.ln_beta = beta; d.ln_eps = eps;
    d.ln_out_bf16 = ln_b; d.ln_out_f32 = ln_f;
    return gemm_desc(A, W, bias, res, C, d);
  }

  int gemm_split(const void* A, int lda, const void* W, void* partials, int M, int N, int K, int split) const {
    vitcap_gemm_desc d = desc(M, N, K, lda, N, VITCAP_ACT_NONE, VITCAP_OUT_F32);
    d.split_k = split;
    return gemm_desc(A, W, nullptr, nullptr, partials, d);
  }

  // Decode-step GEMMs with few rows (M <= 1024), K = 768 or a multiple of it: the 4-stage LDS-DMA ring on small tiles.
  int gemm_ring(const void* A, int lda, const void* W, const float* bias, void* C, int ldc, int M, int N, int K, int act, int out) const {
    vitcap_gemm_desc d = desc(M, N, K, lda, ldc, act, out);
    // 64x32 (32x32 for a handful of rows) tiles.  The ring beats the resident whole-K form (tile_hint 20 / 21) at every batch size
    // once its counted waits are real (docs/LAB_r01_r04.md 4.2 i): decode phase 5.54 -> 5.28 ms at 64 images, 3.84 -> 3.59 at one.
    // K > 768 (`output.dense`, K = 3072): one raw fp32 slab per 768-long k range, summed by vitcap_sum_layernorm (5.24 -> 5.13 ms)
    if (K == 768) d.tile_hint = M <= 32 ? 14 : 13;
    else d.tile_hint = M <= 32 ? 24 : 23;
    return gemm_desc(A, W, bias, nullptr, C, d);
  }

  // x_in: the block's input (read by LN1 and as the residual of proj); x: its output buffer, updated in place from proj on.
  // x_in != x only at the fork (block 8 and tag block 0 both read the output of block 7 and write their own stream), which
  // replaces a 113 MB device-to-device copy of the fork state per batch.
  // have_ln1: `h` already holds norm1(x_in) (written by the previous block's fc2, below).  next: the block that consumes this one's
  // output on the same chain, or null -- its norm1 then rides in this block's fc2 (-> h); norm2 always rides in proj.  Each fused
  // LayerNorm is the separate vitcap_layernorm_fwd launch's arithmetic on the same fp32 rows (vitcap_gemm_desc.ln_*).
  // The dense attention of the encoder blocks (bit0 = 1: encoder key k is cache key k + 1) and of the prefill's visual rows (bit0 = 0):
  // the shipped launch, or under patch removal the KEYMASK instance on this context's rows of the mask.
  int attn_dense(const void* qkv, void* out, int S, int q_rows, int bit0) const {
    if (patch_mask) return vitcap_attn_dense_fwd_keys(qkv, out, B, S, q_rows, 0.125f, patch_mask, MASK_WORDS, bit0, s);
    return q_rows == S ? vitcap_attn_dense_fwd(qkv, out, B, S, 0.125f, s) : vitcap_attn_dense_fwd_rows(qkv, out, B, S, q_rows, 0.125f, s);
  }

  // vitcap_engine_encode_maps: the block's attention probabilities from the qkv buffer its attention launch has just read, into the
  // block's slot of the caller's array (nothing if the block is not selected).  q_rows < NV: the last tag block, CLS query only.
  int emit_block_maps(const vitcap_vit_block_w& bw, const void* qkv, int q_rows) const {
    const bool tag = &bw >= w.tag_blocks && &bw < w.tag_blocks + 4;
    const int bit = tag ? 12 + (int)(&bw - w.tag_blocks) : (int)(&bw - w.blocks);
    if (!(block_maps->mask >> bit & 1)) return VITCAP_OK;
    const int slot = __builtin_popcount(block_maps->mask & ((1u << bit) - 1));
    float* out = block_maps->out + (size_t)slot * B * (block_maps->per_head ? 12 : 1) * NV * NV;
    return vitcap_attn_self_maps(qkv, out, B, NV, q_rows, 0.125f, block_maps->per_head, s);
  }

  int vit_block(const vitcap_vit_block_w& bw, const float* x_in, float* x, void* h, void* qkv, void* mlp, bool have_ln1 = false,
                const vitcap_vit_block_w* next = nullptr) const {
    const int M = B * NV;
    // zz(): each streaming kernel walks the rows the other way round than the one before it (call_state.h: vc_tls_walk_rev); gemm_ln is
    // two launches (GEMM, then the LayerNorm of its rows) and flips between them itself
    if (!have_ln1) { CK(vitcap_layernorm_fwd(x_in, D, bw.n1_g, bw.n1_b, 1e-6f, h, nullptr, M, D, s)); zz(); }
    CK(gemm(h, D, bw.qkv_w, bw.qkv_b, nullptr, 0, qkv, 3 * D, M, 3 * D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));
    zz();
    CK(attn_dense(qkv, h, NV, NV, 1));
    if (block_maps) CK(emit_block_maps(bw, qkv, &bw == &w.tag_blocks[3] ? 1 : NV));      // the last tag block run in full: its CLS row only, as cls_only
    zz();
    // proj reads h (the attention output) as A and its norm2 writes h: a row block's A rows are read by its own three tiles only
    CK(gemm_ln(h, D, bw.proj_w, bw.proj_b, x_in, x, M, D, bw.n2_g, bw.n2_b, 1e-6f, h, nullptr));      // GEMM, LayerNorm: two flips = none
    CK(gemm(h, D, bw.fc1_w, bw.fc1_b, nullptr, 0, mlp, 4 * D, M, 4 * D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_BF16));
    zz();
    if (next) {
      CK(gemm_ln(mlp, 4 * D, bw.fc2_w, bw.fc2_b, x, x, M, 4 * D, next->n1_g, next->n1_b, 1e-6f, h, nullptr));
    } else {
      CK(gemm(mlp, 4 * D, bw.fc2_w, bw.fc2_b, x, D, x, D, M, D, 4 * D, VITCAP_ACT_NONE, VITCAP_OUT_F32));
      zz();
    }
    return VITCAP_OK;
  }

  // The LAST tag block: only row 0 (CLS) of its output is ever read -- the pooler takes tag_hidden[:, 0]
  // (modeling_bert.py:1424) and the joint sequence takes tag_hidden[:, 0] as its first visual token (1493).  So: LN1 and the
  // K/V projections on all 577 rows (the CLS query attends every key), Q / attention / proj / LN2 / MLP for the CLS rows only
  // (strided views of the same buffers: row b*577).  Rows 1..576 of `x` keep the previous block's output.
  int vit_block_cls_only(const vitcap_vit_block_w& bw, float* x, void* h, void* qkv, void* mlp, void* cls_h) const {
    const int M = B * NV;
    const int RS = NV * D;                      // row stride between CLS rows; `h` already holds norm1(x)
    CK(gemm(h, D, (const char*)bw.qkv_w + (size_t)D * D * 2, bw.qkv_b + D, nullptr, 0, (char*)qkv + (size_t)D * 2, 3 * D, M, 2 * D, D,
            VITCAP_ACT_NONE, VITCAP_OUT_BF16));                                         // K | V of every row
    CK(gemm(h, RS, bw.qkv_w, bw.qkv_b, nullptr, 0, qkv, NV * 3 * D, B, D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));   // Q of the CLS rows
    CK(attn_dense(qkv, h, NV, 1, 1));
    if (block_maps) CK(emit_block_maps(bw, qkv, 1));
    CK(gemm(h, RS, bw.proj_w, bw.proj_b, x, RS, x, RS, B, D, D, VITCAP_ACT_NONE, VITCAP_OUT_F32));
    CK(vitcap_layernorm_fwd(x, RS, bw.n2_g, bw.n2_b, 1e-6f, cls_h, nullptr, B, D, s));
    CK(gemm(cls_h, D, bw.fc1_w, bw.fc1_b, nullptr, 0, mlp, 4 * D, B, 4 * D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_BF16));
    CK(gemm(mlp, 4 * D, bw.fc2_w, bw.fc2_b, x, RS, x, RS, B, D, 4 * D, VITCAP_ACT_NONE, VITCAP_OUT_F32));
    return VITCAP_OK;
  }

  // a5 (tag fork) + a6: 4 tag blocks on the forked stream, then the tag head on the tag branch CLS row
  int tag_branch() const {
    float* xt = p<float>(lo.xt);
    const float* xf = p<float>(lo.x);       // fork state (output of block 7)
    for (int i = 0; i < 3; ++i)
      CK(vit_block(w.tag_blocks[i], i == 0 ? xf : xt, xt, ws + lo.th, ws + lo.tqkv, ws + lo.tmlp, i > 0, &w.tag_blocks[i + 1]));
    if (e->full_last_tag_block)
      CK(vit_block(w.tag_blocks[3], xt, xt, ws + lo.th, ws + lo.tqkv, ws + lo.tmlp, true, nullptr));
    else
      CK(vit_block_cls_only(w.tag_blocks[3], xt, ws + lo.th, ws + lo.tqkv, ws + lo.tmlp, ws + lo.pool_in));
    CK(vitcap_gather_rows_bf16(xt, NV, ws + lo.pool_in, B, D, s));
    CK(gemm(ws + lo.pool_in, D, w.pooler_w, w.pooler_b, nullptr, 0, ws + lo.pooled, D, B, D, D, VITCAP_ACT_TANH, VITCAP_OUT_BF16));
    CK(gemm(ws + lo.pooled, D, w.tag_logit.dense_w, w.tag_logit.dense_b, nullptr, 0, ws + lo.tg_f, D, B, D, D, VITCAP_ACT_GELU_ERF,
            VITCAP_OUT_F32));
    CK(vitcap_layernorm_fwd(p<float>(lo.tg_f), D, w.tag_logit.ln_g, w.tag_logit.ln_b, 1e-12f, ws + lo.tg_b, nullptr, B, D, s));
    CK(gemm(ws + lo.tg_b, D, w.tag_logit.dec_w, w.tag_logit.dec_b, nullptr, 0, ws + lo.tag_logits, VP, B, VP, D, VITCAP_ACT_NONE,
            VITCAP_OUT_F32));
    CK(vitcap_sigmoid_topk(p<float>(lo.tag_logits), VP, VITCAP_VOCAB, TOPK, 0.2f, p<int64_t>(lo.tag_ids), p<float>(lo.tag_prob),
                           p<int64_t>(lo.tag_len), B, s));
    return VITCAP_OK;
  }

  int encode_part(const void* image, int image_is_bf16, bool allow_fork) const {
    float* x = p<float>(lo.x);
    // a1: patch embed as GEMM (+bias +pos_embed[1+p]) into rows b*577+1+p; cls rows separately
    CK(vitcap_patch_gather(image, image_is_bf16, ws + lo.patches, B, s));
    vitcap_gemm_desc d = desc(B * 576, D, D, D, D, VITCAP_ACT_NONE, VITCAP_OUT_F32);
    d.ldr = D;
    d.row_group = 576; d.out_group_rows = NV; d.out_row_off = 1; d.res_periodic = 1;
    CK(gemm_desc(ws + lo.patches, w.patch_w, w.patch_b, w.pos_embed + D, x, d));
    zz();
    CK(vitcap_cls_rows(w.cls_token, w.pos_embed, x, B, NV, s));
    // a5: 12 blocks, fork before block 8, 4 tag blocks on the fork.  Run the fork on a side stream when the large GEMMs are
    // in their one-tile-per-workgroup form (batch pipeline) and the batch is small enough for tile-quantisation gaps to
    // matter: B=64 pipelined +2.3 %; with persistent GEMMs or at B=512 it costs 1-2 % (measured), so it stays serial there.
    const bool forked = allow_fork && o.gemm_mode == VITCAP_GEMM_TILES && B <= 128;
    float* x2 = p<float>(lo.x2);
    for (int i = 0; i < 12; ++i) {
      if (i == 8 && forked) {
        // fork: the tag branch depends only on x (the output of block 7), which nobody writes from here on
        CK(ensure_lane(ROLE_SIDE, e->side, e->ev_fork, e->ev_join, "encode: side"));
        CK(fork(s, e->side, e->ev_fork, "encode:"));
        CK(on(e->side).tag_branch());
        CK(ev_record(e->ev_join, e->side, "encode:", "join"));
      }
      // norm1 of block i+1 rides in block i's fc2 (block 7 feeds block 8 that way; the tag branch normalises the fork state itself)
      const vitcap_vit_block_w* next = i + 1 < 12 ? &w.blocks[i + 1] : nullptr;
      if (i < 8) CK(vit_block(w.blocks[i], x, x, ws + lo.h, ws + lo.qkv, ws + lo.mlp, i > 0, next));
      else CK(vit_block(w.blocks[i], i == 8 ? x : x2, x2, ws + lo.h, ws + lo.qkv, ws + lo.mlp, true, next));
    }
    if (forked) return ev_wait(s, e->ev_join, "encode:", "join");
    return tag_branch();
  }

  // the predicted tag tokens as real rows of the joint sequence.  With the mask tensorize_ab builds for a
  // text_b of n tokens (dataset.py:240-252, 387-390) the n tag rows attend each other and the 578 visual rows, and every caption
  // row attends them; nothing they attend depends on the caption, so their hidden states -- hence their K/V in every decoder
  // layer -- are computed ONCE here, for BOTH embedding branches of modeling_bert.py:1435-1489 (the reference re-evaluates
  // `topk_len[0] + 20 <= L` at every step: the decode attention picks the branch per step, vitcap_attn_decode_step_tags).
  // Per layer: tag q|k|v (compact rows = the cache) -> joint buffer [visual K/V | tag rows] per image -> dense MFMA attention on
  // the query range that covers the tag rows -> BertSelfOutput / BertIntermediate / BertOutput on the tag rows.
  int prefill_tags() const {
    const int n = lo.NT, R = B * n, S2 = SV + n;
    if (!o.tagemb_cls && !(w.xword_emb && w.xpos_emb && w.xtype_emb && w.xemb_ln_g && w.xemb_ln_b)) {
      vitcap_set_error("prefill: tag_visible with tagemb != 'cls' needs bert.extra_embeddings bound (vitcap_weights.x*)");
      return VITCAP_ESTATE;
    }
    for (int v = 0; v < 2; ++v)
      CK(vitcap_tag_embed(p<int64_t>(lo.tag_ids), n, o.tag_pos0, v == 0, o.tagemb_cls, w.cls.dec_w, w.word_emb, w.pos_emb, w.type_emb,
                          w.emb_ln_g, w.emb_ln_b, w.xword_emb, w.xpos_emb, w.xtype_emb, w.xemb_ln_g, w.xemb_ln_b, 1e-12f,
                          p<float>(lo.tagx_f(v)), p(lo.tagx_b(v)), B, s));
    for (int l = 0; l < 4; ++l) {
      const vitcap_bert_layer_w& lw = w.dec[l];
      if (l < 3)        // visual K | V of this layer into the joint buffer (the Q columns of those rows are never read as queries we keep)
        CK(vitcap_copy_row_blocks(ws + lo.dqkv[l], SV, 0, 3 * D, D, ws + lo.jqkv, JROWS, 0, 3 * D, D, SV, 2 * D, B, s));
      for (int v = 0; v < 2; ++v) {
        char* tq = p(lo.tqkv_c(v, l));
        float* xf = p<float>(lo.tagx_f(v));
        char* xb = p(lo.tagx_b(v));
        if (l == 3) {   // the last layer's tag-row outputs feed nothing: K | V only
          CK(gemm(xb, D, (const char*)lw.qkv_w + (size_t)D * D * 2, lw.qkv_b + D, nullptr, 0, tq + (size_t)D * 2, 3 * D, R, 2 * D, D,
                  VITCAP_ACT_NONE, VITCAP_OUT_BF16));
          continue;
        }
        CK(gemm(xb, D, lw.qkv_w, lw.qkv_b, nullptr, 0, tq, 3 * D, R, 3 * D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));
        CK(vitcap_copy_row_blocks(tq, n, 0, 3 * D, 0, ws + lo.jqkv, JROWS, SV, 3 * D, 0, n, 3 * D, B, s));
        CK(vitcap_attn_dense_fwd_train_rows(ws + lo.jqkv, ws + lo.jout, p<float>(lo.jlse), B, S2, JROWS, 0.125f, 0.f, 0u, 0, 0, 512, S2, s));
        CK(vitcap_copy_row_blocks(ws + lo.jout, JROWS, SV, D, 0, ws + lo.tg_ctx, n, 0, D, 0, n, D, B, s));
        CK(gemm(ws + lo.tg_ctx, D, lw.ao_w, lw.ao_b, xf, D, ws + lo.tg_tmp, D, R, D, D, VITCAP_ACT_NONE, VITCAP_OUT_F32));
        CK(vitcap_layernorm_fwd(p<float>(lo.tg_tmp), D, lw.ao_g, lw.ao_beta, 1e-12f, ws + lo.tg_sa_b, p<float>(lo.tg_sa_f), R, D, s));
        CK(gemm(ws + lo.tg_sa_b, D, lw.i_w, lw.i_b, nullptr, 0, ws + lo.tg_mlp, 4 * D, R, 4 * D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_BF16));
        CK(gemm(ws + lo.tg_mlp, 4 * D, lw.o_w, lw.o_b, p<float>(lo.tg_sa_f), D, ws + lo.tg_tmp, D, R, D, 4 * D, VITCAP_ACT_NONE,
                VITCAP_OUT_F32));
        CK(vitcap_layernorm_fwd(p<float>(lo.tg_tmp), D, lw.o_g, lw.o_beta, 1e-12f, xb, xf, R, D, s));
      }
    }
    return VITCAP_OK;
  }

  int prefill_part() const {
    const int M = B * SV;
    float* vis_f = p<float>(lo.vis_f);
    void* vis_b = ws + lo.vis_b;
    CK(vitcap_assemble_visual(p<float>(lo.x2), p<float>(lo.xt), vis_f, vis_b, B, NV, s));
    for (int l = 0; l < 4; ++l) {
      const vitcap_bert_layer_w& lw = w.dec[l];
      void* dq = ws + lo.dqkv[l];
      if (l == 3) {        // the last layer's visual-row outputs feed nothing: only its K/V are needed (no Q either)
        CK(gemm(vis_b, D, (const char*)lw.qkv_w + (size_t)D * D * 2, lw.qkv_b + D, nullptr, 0, (char*)dq + (size_t)D * 2, 3 * D, M,
                2 * D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));
        if (lo.vt[l]) CK(vitcap_attn_beam_vt(dq, ws + lo.vt[l], B, SV, s));
        break;
      }
      CK(gemm(vis_b, D, lw.qkv_w, lw.qkv_b, nullptr, 0, dq, 3 * D, M, 3 * D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));
      zz();
      if (lo.vt[l]) CK(vitcap_attn_beam_vt(dq, ws + lo.vt[l], B, SV, s));
      CK(attn_dense(dq, ws + lo.h, SV, SV, 0));
      zz();
      // BertSelfOutput / BertOutput: dense + residual, then LayerNorm (post-LN)
      CK(gemm_ln(ws + lo.h, D, lw.ao_w, lw.ao_b, vis_f, ws + lo.dtmp, M, D, lw.ao_g, lw.ao_beta, 1e-12f, ws + lo.da_b, p<float>(lo.da_f)));
      CK(gemm(ws + lo.da_b, D, lw.i_w, lw.i_b, nullptr, 0, ws + lo.mlp, 4 * D, M, 4 * D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_BF16));
      zz();
      CK(gemm_ln(ws + lo.mlp, 4 * D, lw.o_w, lw.o_b, p<float>(lo.da_f), ws + lo.dtmp, M, 4 * D, lw.o_g, lw.o_beta, 1e-12f, vis_b, vis_f));
    }
    if (lo.NT > 0) CK(prefill_tags());
    return VITCAP_OK;
  }

  // vitcap_gen_opts.encode_parts: the batch is cut into parts whose encoder + prefill run as independent chains on separate
  // streams (part 0 on the caller's), so that the tile-quantisation tail of one part's GEMM (qkv: 5.1 rounds of 256 CUs cost 6 at
  // B = 64) is filled by the other part's kernels; every row's arithmetic is unchanged (bit-identical results).  Measured,
  // 2-slot pipeline, images/s without / with 2 parts: B = 16 2039 / 2034, 32 2825 / 2854, 64 3560 / 3635, 128 3724 / 3808,
  // 512 3975 / 3990; 3 and 4 parts lose (B = 64: 3318 / 3460).  With two GEMM chains in flight every launch of the dominant kernel
  // shares the chip with the other chain: its per-launch rate (the bench's roofline.frac) drops from 0.24 to 0.17 of peak although
  // throughput rises -- roofline.frac_busy (flops / union of the launches' intervals) is the figure that stays comparable.
  // VITCAP_ENCODE_SPLIT overrides for experiments.
  int encode_parts() const {
    static const int env = [] { const char* v = getenv("VITCAP_ENCODE_SPLIT"); return v ? atoi(v) : -1; }();
    int np = env >= 0 ? env : o.encode_parts;
    // auto (round 5): two parts inside the batch pipeline from 32 images on -- images/s is the metric (+2.1 % at B = 64, +2.3 % at 128,
    // +0.4 % at 512, measured above); the bench reports the dominant kernel's busy-interval rate (frac_busy) beside the per-launch one
    if (np == 0) np = (o.gemm_mode == VITCAP_GEMM_TILES && B >= 32) ? 2 : 1;
    if (np > 4) np = 4;
    if (B < 8 || lo.NT > 0) np = 1;
    return np;
  }

  int encode(const void* image, int image_is_bf16) const {
    if (!image) { vitcap_set_error("encode: null image"); return VITCAP_EINVAL; }
    // timing runs: a step is sampled WHOLE (its encoder and prefill launches), so that the union of the sampled launches' intervals
    // still sees which of them ran next to each other (tag branch beside caption blocks 8-11, batch parts)
    if (e->timing) e->timing_this_step = (e->timing_seen++ % e->timing_stride) == 0;
    const int np = encode_parts();
    if (np < 2) return encode_part(image, image_is_bf16, true);
    for (int i = 0; i < np - 1; ++i) CK(ensure_lane(ROLE_PART0 + i, e->part[i], e->ev_pfork, e->ev_pjoin[i], "encode: part"));
    CK(ev_record(e->ev_pfork, s, "encode: split", "fork"));
    const size_t img_bytes = (size_t)3 * 384 * 384 * (image_is_bf16 ? 2 : 4);
    int i0[5];
    for (int i = 0; i <= np; ++i) i0[i] = (int)((long long)B * i / np);
    Layout lv[4];
    for (int i = 0; i < np; ++i) lv[i] = lo.from_image(i0[i]);
    auto part = [&](int i) { return view(lv[i], i0[i + 1] - i0[i], i == 0 ? s : (void*)e->part[i - 1], i0[i]); };
    for (int i = 0; i < np; ++i) {
      if (i > 0) CK(ev_wait(part(i).s, e->ev_pfork, "encode: split", "fork"));
      CK(part(i).encode_part((const char*)image + (size_t)i0[i] * img_bytes, image_is_bf16, false));
    }
    // the prefill of each part follows on its own stream (prefill() then has nothing left to do)
    for (int i = 0; i < np; ++i) {
      CK(part(i).prefill_part());
      if (i > 0) CK(join(part(i).s, s, e->ev_pjoin[i - 1], "encode: split"));
    }
    return VITCAP_OK;
  }

  int prefill() const {
    if (encode_parts() >= 2) return VITCAP_OK;       // done by encode(), per part
    return prefill_part();
  }

  // One decode step for the sequences of `pt` (K sequences share one image's visual K/V): embeddings of (token t-1, [MASK]) ->
  // 4 decoder layers against the caches -> LM head on the [MASK] rows -> fp32 logits [ns, VOCAB_PAD] (+ row statistics).
  int step_forward(int t, const int64_t* ids_all, char* tcache, bool embed, bool rowstat, const Part& pt) const {
    const int NS = lo.NS, K = lo.K, L = lo.L;
    const int ns = pt.ns, R = 2 * ns;      // two step-buffer rows per sequence
    const size_t s0 = (size_t)pt.s0, i0 = (size_t)pt.i0;
    float* xs_f = p<float>(lo.xs_f, s0);
    char* xs_b = p(lo.xs_b, s0);
    char* sqkv = p(lo.sqkv, s0);
    char* sctx = p(lo.sctx, s0);
    float* sa_f = p<float>(lo.sa_f, s0);
    char* sa_b = p(lo.sa_b, s0);
    char* smlp = p(lo.smlp, s0);
    char* hd_b = p(lo.hd_b, s0);
    float* slab = p<float>(lo.spart, s0);      // the slice's own slab region
    if (embed)          // otherwise the previous step's vitcap_greedy_select_embed already wrote this step's x
      CK(vitcap_embed_step(ids_all + s0 * L, L, t, o.mask_token_id, w.word_emb, w.pos_emb, w.type_emb, w.emb_ln_g, w.emb_ln_b, 1e-12f,
                           xs_f, xs_b, ns, s));
    // small-tile LDS-DMA ring kernels (gemm_ring) for batches of few rows; larger ones take the big-tile / split-K path.  The choice
    // follows the WHOLE batch, so that a sequence's arithmetic does not depend on how the batch is sliced.
    // up to 1024 rows (512 sequences) the small-tile ring forms of gemm_ring win (decode phase 13.2 -> 11.9 ms at 256 images,
    // 20.4 -> 19.9 at 512); at 2560 rows (5 beams x 256 images) the 128x128 / 256x256 tiles do (21.4 against 23.8 ms)
    const bool small = 2 * NS <= 1024;
    // the slice's R rows, K = 768 -> bf16 [R, N] with bias (and activation): qkv and intermediate.dense
    auto proj = [&](const void* A, const void* W, const float* bias, void* C, int N, int act) {
      return small ? gemm_ring(A, D, W, bias, C, N, R, N, D, act, VITCAP_OUT_BF16)
                   : gemm(A, D, W, bias, nullptr, 0, C, N, R, N, D, act, VITCAP_OUT_BF16);
    };
    // M rows -> raw fp32 partial slabs [M, 768] for vitcap_sum_layernorm, which reduces them inside the fused bias + residual +
    // LayerNorm kernel: attention.output.dense, output.dense (BertSelfOutput / BertOutput, modeling_bert.py:353-357, 415-419) and
    // the LM head's transform.  Returns in `split` how many: the ring writes one per 768-long k range, the big tiles `split` as given.
    auto slabs = [&](const void* A, int lda, const void* W, int M, int Kd, int& split) {
      if (!small) return gemm_split(A, lda, W, slab, M, D, Kd, split);
      split = Kd / D;
      return gemm_ring(A, lda, W, nullptr, slab, D, M, D, Kd, VITCAP_ACT_NONE, VITCAP_OUT_F32);
    };
    // split-K of the N = 768 GEMMs by the WHOLE batch's rows (a sequence's sums must not depend on how the batch is sliced):
    // 6 / 12 slabs fill the chip at a few hundred rows; from ~1000 rows on the output tiles alone do, and the fp32 slabs (47 /
    // 94 MB per GEMM at 2560 rows) cost more than they buy -- decode phase at 5 beams x 256 images 24.6 -> 22.0 ms, 512 greedy
    // sequences 21.5 -> 20.8 ms, 256 sequences unchanged (measured)
    const int rows_all = 2 * NS;
    const int split_ao = rows_all >= 2048 ? 1 : (rows_all >= 1024 ? 2 : SPLIT_AO), split_fc2 = rows_all >= 1024 ? 4 : SPLIT_FC2;
    const int split_hd = NS >= 2048 ? 1 : (NS >= 1024 ? 2 : SPLIT_AO);      // as above, by the whole batch's [MASK] rows
    for (int l = 0; l < 4; ++l) {
      const vitcap_bert_layer_w& lw = w.dec[l];
      char* tc = tcache + lo.tcache_at(l, s0);
      const char* vis = p(lo.dqkv[l], i0);
      CK(proj(xs_b, lw.qkv_w, lw.qkv_b, sqkv, 3 * D, VITCAP_ACT_NONE));
      if (vis_mask && lo.vt[l] && K >= 2 && K <= 8)
        // beam search with a mask (vitcap_engine_decode_beam_masked): one row per IMAGE, a slice starts at its first image's row
        CK(vitcap_attn_decode_beam_groups_masked(sqkv, vis, p(lo.vt[l], i0), tc, sctx, ns / K, K, 1, SV, t, L, 0.125f,
                                                 vis_mask + (size_t)i0 * MASK_WORDS, MASK_WORDS, s));
      else if (vis_mask)      // a slice starts at its first sequence's row
        CK(vitcap_attn_decode_step_masked(sqkv, vis, tc, sctx, ns, SV, t, L, K, 0.125f, vis_mask + s0 * MASK_WORDS, MASK_WORDS, s));
      else if (lo.NT > 0)
        CK(vitcap_attn_decode_step_tags(sqkv, vis, tc, sctx, ns, SV, t, L, K, 0.125f, p(lo.tqkv_c(0, l), i0), p(lo.tqkv_c(1, l), i0), lo.NT,
                                        p<int64_t>(lo.tag_len), s));
      else if (lo.vt[l] && K >= 2 && K <= 8)
        // several sequences per image (beam search): all of an image's query rows against its visual rows on the matrix pipe
        CK(vitcap_attn_decode_beams(sqkv, vis, p(lo.vt[l], i0), tc, sctx, ns / K, K, SV, t, L, 0.125f, s));
      else if (lo.vt[l] && K > 8 && lo.group_k > 1)
        // more than 8 sequences per image (constrained beam search: states x beams): groups of group_k sequences, K / group_k per image
        CK(vitcap_attn_decode_beam_groups(sqkv, vis, p(lo.vt[l], i0), tc, sctx, ns / K, lo.group_k, K / lo.group_k, SV, t, L, 0.125f, s));
      else
        CK(vitcap_attn_decode_step(sqkv, vis, tc, sctx, ns, SV, t, L, K, 0.125f, s));
      int n_ao = split_ao, n_fc2 = split_fc2;
      CK(slabs(sctx, D, lw.ao_w, R, D, n_ao));
      CK(vitcap_sum_layernorm(slab, n_ao, (size_t)R * D, lw.ao_b, xs_f, D, 0, lw.ao_g, lw.ao_beta, 1e-12f, sa_b, sa_f, R, D, s));
      CK(proj(sa_b, lw.i_w, lw.i_b, smlp, 4 * D, VITCAP_ACT_GELU_ERF));
      CK(slabs(smlp, 4 * D, lw.o_w, R, 4 * D, n_fc2));
      CK(vitcap_sum_layernorm(slab, n_fc2, (size_t)R * D, lw.o_b, sa_f, D, 0, lw.o_g, lw.o_beta, 1e-12f, xs_b, xs_f, R, D, s));
    }
    // LM head on the [MASK] rows (row 1 of every pair): A = xs_b + 768, lda = 1536
    int n_hd = split_hd;
    CK(slabs(xs_b + D * 2, 2 * D, w.cls.dense_w, ns, D, n_hd));
    CK(vitcap_sum_layernorm(slab, n_hd, (size_t)ns * D, w.cls.dense_b, nullptr, 0, 1, w.cls.ln_g, w.cls.ln_b, 1e-12f, hd_b, nullptr, ns, D, s));
    // vocabulary GEMM: 47 MB of weights streamed once per step.  With few rows (greedy: NS <= 128) the 64x64-tile kernel
    // moves them at 3.8 TB/s against 2.3 TB/s for the 32x32 tiles the small-M dispatch would pick (12.5 vs 20.8 us at NS = 64)
    vitcap_gemm_desc d = desc(ns, VP, D, D, VP, VITCAP_ACT_NONE, VITCAP_OUT_F32);
    d.tile_hint = NS <= 128 ? 1 : 0;
    d.rowstat = rowstat ? p<float>(lo.rowstat, s0) : nullptr;      // greedy: argmax / log-softmax pieces next to the logits
    return gemm_desc(hd_b, w.cls.dec_w, w.cls.dec_b, nullptr, p(lo.logits, s0), d);
  }

  // Greedy / sampled decode loop of NS = B * K sequences, K per image (K > 1: ViTCAP.generate with num_return_sequences = K
  // expands every input K times, modeling_bert.py:976-994; the K copies of an image share its encoder output and visual K/V
  // here, as the beams of a beam search do).  Results stay in the workspace (lo.ids, lo.logprob, lo.last_tok).
  int greedy_loop() const {
    const int NS = lo.NS, L = lo.L, K = lo.K;
    CK(vitcap_greedy_init(p<int64_t>(lo.ids), p<int32_t>(lo.unf), p<float>(lo.sum_lp), p<float>(lo.cnt), NS, L, o.bos_token_id,
                          o.pad_token_id, s));
    if (forced >= 0)      // the step kernels write the positions a sequence takes a token at; column 0 and what lies behind its end stay 0
      HIPCK(hipMemsetAsync(ws + lo.tok_lp, 0, (size_t)NS * lo.tok_lp.unit, (hipStream_t)s), "decode: token log-probs clear");
    // Plain greedy decoding of a small batch: the vocabulary GEMM also emits per-piece (max, argmax, sum exp) of its rows, and ONE
    // kernel turns them into the token, its log-prob, the bookkeeping and the NEXT step's embedded rows -- instead of reading the
    // 30522-wide fp32 rows back (greedy_step 18.7 us) and a separate embedding launch per step.
    const bool fused = !o.sampling.do_sample && o.repetition_penalty == 1.0f && NS <= 128;
    // two slices on two streams (decode_streams = 2): measured at 64 sequences, eager and graph-replayed: 5.96 ms per batch against
    // 5.66 ms for one chain -- the ~4.5 us per dependent small kernel is not hidden by a second chain (the dispatch path is the
    // shared resource), so auto = 1; the option stays for experiments and is covered by tests (bit-identical results)
    const int nparts = o.decode_streams == 2 && B >= 2 ? 2 : 1;
    Part parts[2] = {{0, NS, 0}, {0, 0, 0}};
    if (nparts == 2) {
      const int b0 = B / 2;
      parts[0] = Part{0, b0 * K, 0};
      parts[1] = Part{b0 * K, (B - b0) * K, b0};
      CK(ensure_lane(ROLE_DEC2, e->dec2, e->ev_dfork, e->ev_djoin, "decode: second"));
      CK(fork(s, e->dec2, e->ev_dfork, "decode:"));
    }
    const Enq second = on(nparts == 2 ? (void*)e->dec2 : s);
    for (int t = 1; t < L; ++t) {
      for (int i = 0; i < nparts; ++i) {            // the slices' launches alternate so that both streams are fed evenly
        const Part& pt = parts[i];
        const Enq& q = i == 0 ? *this : second;
        const size_t s0 = (size_t)pt.s0;
        CK(q.step_forward(t, p<int64_t>(lo.ids), ws + lo.tcache, !fused || t == 1, fused, pt));
        int64_t* ids = p<int64_t>(lo.ids, s0);
        int32_t* unf = p<int32_t>(lo.unf, s0);
        float *sum_lp = p<float>(lo.sum_lp, s0), *cnt = p<float>(lo.cnt, s0), *logprob = p<float>(lo.logprob, s0);
        float *logits = p<float>(lo.logits, s0), *margins = p<float>(lo.margins, s0);
        int64_t* last_tok = p<int64_t>(lo.last_tok, s0);
        // a plain call hands the step kernels nulls, which is what the entry points without `_forced` do
        const int64_t* fids = forced >= 0 ? p<int64_t>(lo.forced, s0) : nullptr;
        float* tok_lp = forced >= 0 ? p<float>(lo.tok_lp, s0) : nullptr;
        const int sf = forced > 0 ? 1 : 0;
        if (fused) {
          CK(vitcap_greedy_select_embed_forced(p<float>(lo.rowstat, s0), RS_PIECES, logits, VP, VITCAP_VOCAB, ids, unf, sum_lp, cnt,
                                               logprob, last_tok, pt.ns, t, L, o.eos_token_id, o.pad_token_id, o.mask_token_id,
                                               w.word_emb, w.pos_emb, w.type_emb, w.emb_ln_g, w.emb_ln_b, 1e-12f, p<float>(lo.xs_f, s0),
                                               p(lo.xs_b, s0), fids, sf, tok_lp, q.s));
          continue;
        }
        if (o.repetition_penalty != 1.0f)
          CK(vitcap_repetition_penalty(logits, VP, VITCAP_VOCAB, ids, L, t, o.repetition_penalty, pt.ns, q.s));
        if (o.sampling.do_sample) {
          // the draws are keyed by (seed, sequence index within the call): a slice passes its first sequence as the stream offset
          vitcap_sample_params sp = o.sampling;
          CK(vitcap_sample_step_forced(logits, VP, VITCAP_VOCAB, ids, unf, sum_lp, cnt, logprob, margins, last_tok, pt.ns, t, L,
                                       o.eos_token_id, o.pad_token_id, &sp, pt.s0, fids, sf, tok_lp, q.s));
        } else {
          CK(vitcap_greedy_step_forced(logits, VP, VITCAP_VOCAB, ids, unf, sum_lp, cnt, logprob, margins, last_tok, pt.ns, t, L,
                                       o.eos_token_id, o.pad_token_id, fids, sf, tok_lp, q.s));
        }
      }
    }
    if (nparts == 2) CK(join(e->dec2, s, e->ev_djoin, "decode:"));
    return VITCAP_OK;
  }

  // beam search and CBS: the text K/V history (positions 0..t-1) follows the back-pointers into the other cache for the next step
  int follow_parents(char*& cur, char*& alt, const int32_t* parent, int t) const {
    if (t + 1 >= lo.L) return VITCAP_OK;
    CK(vitcap_beam_reorder_cache(cur, alt, parent, 4, lo.NS, lo.L, t, s));
    std::swap(cur, alt);
    return VITCAP_OK;
  }

  // Beam search loop (a13): B*beams sequences, all bookkeeping on device; the final n-best lists land in lo.fin_ids / lo.fin_lp.
  int beam_loop() const {
    const int NS = lo.NS, L = lo.L, beams = o.num_beams;
    vitcap_beam_state st;
    st.ids_in = p<int64_t>(lo.ids);
    st.ids_out = p<int64_t>(lo.ids2);
    st.beam_scores = p<float>(lo.beam_scores);
    st.parent = p<int32_t>(lo.parent);
    st.done = p<int32_t>(lo.done);
    st.has_hyp = p<int32_t>(lo.has_hyp);
    st.hyp_score = p<float>(lo.hyp_score);
    st.hyp_len = p<int32_t>(lo.hyp_len);
    st.hyp_tok = p<int64_t>(lo.hyp_tok);
    st.n_keep = o.num_keep_best;
    CK(vitcap_beam_init(&st, B, beams, L, o.bos_token_id, o.pad_token_id, s));
    char* tc_cur = ws + lo.tcache;
    char* tc_alt = ws + lo.tcache2;
    float *logits = p<float>(lo.logits), *cand_val = p<float>(lo.cand_val), *lse = p<float>(lo.lse);
    int32_t* cand_idx = p<int32_t>(lo.cand_idx);
    const int C = 2 * beams;
    // plain beam search: the candidates come from the vocabulary GEMM's row statistics (the 30522-wide rows are not read back:
    // row_topk_lse 139 us -> 12 us per step at 256 images x 5 beams); with a repetition penalty the logits change after the
    // GEMM, and the sampled form draws from the whole filtered row, so both keep the row scan
    const bool from_pieces = !o.sampling.do_sample && o.repetition_penalty == 1.0f;
    for (int t = 1; t < L; ++t) {
      CK(step_forward(t, st.ids_in, tc_cur, true, from_pieces, Part{0, NS, 0}));
      if (o.repetition_penalty != 1.0f)
        CK(vitcap_repetition_penalty(logits, VP, VITCAP_VOCAB, st.ids_in, L, t, o.repetition_penalty, NS, s));
      if (o.sampling.do_sample) {   // modeling_utils.py:966-985: two sampled words per beam instead of the 2*beams best
        CK(vitcap_beam_sample_candidates(logits, VP, VITCAP_VOCAB, NS, t, &o.sampling, 0, cand_val, cand_idx, lse, s));
        CK(vitcap_beam_step_sampled(cand_val, cand_idx, lse, &st, B, beams, VITCAP_VOCAB, t, L, o.eos_token_id, o.pad_token_id,
                                    o.length_penalty, s));
      } else {
        if (from_pieces)
          CK(vitcap_row_topk_pieces(logits, VP, VITCAP_VOCAB, p<float>(lo.rowstat), RS_PIECES, C, cand_val, cand_idx, lse, NS, s));
        else
          CK(vitcap_row_topk_lse(logits, VP, VITCAP_VOCAB, C, cand_val, cand_idx, lse, NS, s));
        CK(vitcap_beam_step(cand_val, cand_idx, lse, &st, B, beams, VITCAP_VOCAB, t, L, o.eos_token_id, o.pad_token_id, o.length_penalty, s));
      }
      CK(follow_parents(tc_cur, tc_alt, st.parent, t));
      std::swap(st.ids_in, st.ids_out);
    }
    // finalize reads hypotheses only; it runs whether or not the loop ended early
    return vitcap_beam_finalize(&st, p<int64_t>(lo.fin_ids), p<float>(lo.fin_lp), B, L, o.eos_token_id, o.pad_token_id, s);
  }

  // Constrained beam search loop (ViTCAP.generate with use_cbs, modeling_bert.py:1035-1057): B * S * num_beams
  // sequences through the same decode step as beam search, bookkeeping of utils_cbs.py:26-443 on the device (csrc/cbs.hip).  The
  // reference re-runs the whole model on every prefix (`state` stays None); here the text K/V caches follow the back-pointers.
  int cbs_loop() const {
    const int NS = lo.NS, L = lo.L, S = o.cbs_states, K = o.num_beams;
    vitcap_cbs_state st;
    st.ids_in = p<int64_t>(lo.ids);
    st.ids_out = p<int64_t>(lo.ids2);
    st.scores_in = p<float>(lo.cbs_sc);
    st.scores_out = p<float>(lo.cbs_sc2);
    st.parent = p<int32_t>(lo.cbs_parent);
    st.unfinished = p<int32_t>(lo.cbs_unf);
    st.n_pred = p<int32_t>(lo.cbs_npred);
    st.live = p<int32_t>(lo.live);
    CK(vitcap_cbs_init(&st, B, S, K, L, o.bos_token_id, s));
    CK(vitcap_cbs_pair_flags(o.fsm, B, S, VITCAP_VOCAB, p<uint8_t>(lo.cbs_flags), s));
    char* tc_cur = ws + lo.tcache;
    char* tc_alt = ws + lo.tcache2;
    const float* logits = p<float>(lo.logits);
    float* lse = p<float>(lo.cbs_lse);
    for (int t = 1; t < L; ++t) {
      CK(step_forward(t, st.ids_in, tc_cur, true, false, Part{0, NS, 0}));
      CK(vitcap_row_topk_lse(logits, VP, VITCAP_VOCAB, 1, p<float>(lo.cbs_max), p<int32_t>(lo.cbs_argmax), lse, NS, s));
      if (t == 1) {
        CK(vitcap_cbs_start(logits, VP, VITCAP_VOCAB, lse, o.fsm, &st, B, S, K, L, o.eos_token_id, o.eos_extra, s));
      } else {
        CK(vitcap_cbs_candidates(logits, VP, VITCAP_VOCAB, lse, o.fsm, &st, B, S, K, t, L, o.eos_token_id, o.eos_extra, o.cbs_no_repeat,
                                 o.cbs_bad_ending, p<uint8_t>(lo.cbs_flags), p<float>(lo.cbs_val), p<int32_t>(lo.cbs_word), s));
        CK(vitcap_cbs_select(p<float>(lo.cbs_val), p<int32_t>(lo.cbs_word), &st, B, S, K, t, L, o.eos_token_id, o.eos_extra, s));
      }
      CK(follow_parents(tc_cur, tc_alt, st.parent, t));
      std::swap(st.ids_in, st.ids_out);
      std::swap(st.scores_in, st.scores_out);
    }
    return vitcap_cbs_finalize(&st, o.num_constraints, o.min_constraints_to_satisfy, B, S, K, L, o.eos_token_id, o.eos_extra, o.pad_token_id,
                               p<int64_t>(lo.cbs_fin_ids), p<float>(lo.cbs_fin_lp), s);
  }

  int decode_loop() const {
    if (lo.cbs) return cbs_loop();
    return lo.beam ? beam_loop() : greedy_loop();
  }

 private:
  Enq(const Enq& q, const Layout& lv, int Bv, void* sv, int first_image)
      : e(q.e), w(q.w), o(q.o), lo(lv), ws(q.ws), B(Bv), s(sv), live(q.live), owner(false), forced(q.forced), vis_mask(q.vis_mask),
        patch_mask(q.patch_mask ? q.patch_mask + (size_t)first_image * MASK_WORDS : nullptr) {}      // block_maps stays null: vitcap_engine_encode_maps runs no views (its slots are laid out for the whole batch)
};

vitcap_gen_opts opts_or_default(const vitcap_gen_opts* opts) { return opts ? *opts : default_opts(); }

// What every enqueueing entry point does before it takes the engine's lock: validate the options, lay the workspace out, check the
// engine and the workspace against it.
int enter(vitcap_engine* e, int B, const vitcap_gen_opts& o, void* ws, size_t ws_bytes, Layout& lo) {
  if (B <= 0 || check_opts(o) != VITCAP_OK) { if (B <= 0) vitcap_set_error("engine: bad batch"); return VITCAP_EINVAL; }
  lo = Layout(B, o);
  if (!e || !e->bound) { vitcap_set_error("engine: weights not bound"); return VITCAP_ESTATE; }
  if (!ws) { vitcap_set_error("engine: bad batch/workspace"); return VITCAP_EINVAL; }
  if (((uintptr_t)ws & 255) != 0) { vitcap_set_error("engine: workspace must be 256-byte aligned"); return VITCAP_EINVAL; }
  if (ws_bytes < lo.off) {
    vitcap_set_error("engine: workspace %zu < required %zu bytes", ws_bytes, lo.off);
    return VITCAP_EWORKSPACE;
  }
  return VITCAP_OK;
}

// What the `_forced` entry points add to a decode call; a plain call passes the default.
struct Forced {
  const int64_t* ids = nullptr;     // device [NS][L] or null
  int score = 0;
  float* out_tok_lp = nullptr;      // device [NS][L] or null
  const uint32_t* vis_mask = nullptr;      // the `_masked` entry points: device [NS][MASK_WORDS], read in place
  bool masked = false;
  bool on() const { return ids || out_tok_lp; }
};
// what a visibility mask is not built for: refused by the option's name before anything is enqueued
int check_masked(const vitcap_gen_opts& o, const Forced& f) {
  if (check_opts(o) != VITCAP_OK) return VITCAP_EINVAL;
  const char* bad = nullptr;
  if (o.num_beams > 1) bad = "num_beams > 1";
  else if (o.use_cbs) bad = "use_cbs";
  else if (o.tag_visible > 0) bad = "tag_visible > 0";
  else if (o.use_graph) bad = "use_graph = 1 (a captured loop would freeze this call's mask pointer)";
  if (bad) { vitcap_set_error("masked decoding: a visibility mask is not built for %s", bad); return VITCAP_EINVAL; }
  if (!f.vis_mask) { vitcap_set_error("masked decoding: vis_mask is null"); return VITCAP_EINVAL; }
  if (((uintptr_t)f.vis_mask & 3) != 0) { vitcap_set_error("masked decoding: vis_mask is not 4-byte aligned"); return VITCAP_EINVAL; }
  return VITCAP_OK;
}
// the beam counterpart (vitcap_engine_decode_beam_masked): one mask row per image, 2..8 beams; refused by name before anything else
int check_beam_masked(const vitcap_gen_opts& o, const Forced& f) {
  if (check_opts(o) != VITCAP_OK) return VITCAP_EINVAL;
  const char* bad = nullptr;
  if (o.num_beams < 2 || o.num_beams > 8) bad = "num_beams outside 2..8 (num_beams == 1 is vitcap_engine_decode_masked)";
  else if (o.use_cbs) bad = "use_cbs";
  else if (o.tag_visible > 0) bad = "tag_visible > 0";
  else if (o.sampling.do_sample) bad = "do_sample (beam sampling)";
  else if (o.use_graph) bad = "use_graph = 1 (a captured loop would freeze this call's mask pointer)";
  else if (f.on()) bad = "forced_ids / token_logprobs (forced tokens under beam search)";
  if (bad) { vitcap_set_error("masked beam decoding: a visibility mask under beam search is not built for %s", bad); return VITCAP_EINVAL; }
  if (!f.vis_mask) { vitcap_set_error("masked beam decoding: vis_mask is null"); return VITCAP_EINVAL; }
  if (((uintptr_t)f.vis_mask & 3) != 0) { vitcap_set_error("masked beam decoding: vis_mask is not 4-byte aligned"); return VITCAP_EINVAL; }
  return VITCAP_OK;
}
// forced tokens are built for the greedy / sampling loop only: refused by name before anything is enqueued
int check_forced(const vitcap_gen_opts& o, const Forced& f) {
  if (!f.on()) return VITCAP_OK;
  if (check_opts(o) != VITCAP_OK) return VITCAP_EINVAL;
  if (o.num_beams > 1 || o.use_cbs) {
    vitcap_set_error("forced decoding: forced_ids / token_logprobs need num_beams == 1 and no constrained beam search (got num_beams=%d, "
                     "use_cbs=%d); forced tokens under beam search are not built", o.num_beams, o.use_cbs);
    return VITCAP_EINVAL;
  }
  if (f.score != 0 && f.score != 1) { vitcap_set_error("forced decoding: score_forced must be 0 or 1 (got %d)", f.score); return VITCAP_EINVAL; }
  return VITCAP_OK;
}

int decode_locked(vitcap_engine* e, int B, const vitcap_gen_opts& o, const Layout& lo, char* ws, int64_t* out_ids, float* out_logprobs,
                  int64_t* out_last_tok, void* s, const Forced& f = Forced()) {
  if (!out_ids || !out_logprobs) { vitcap_set_error("decode: null outputs"); return VITCAP_EINVAL; }
  hipStream_t st = (hipStream_t)s;
  const bool graph = o.use_graph && !o.sampling.do_sample && !f.masked;      // check_masked has refused use_graph with a mask
  const int fmode = f.on() ? f.score : -1;
  // The loop -- eager or replayed -- reads the forced ids from the workspace, never from the caller's array: a captured loop holds
  // no pointer of the call it was captured in.  No ids given (only the per-token log-probs are wanted): every entry -1.
  if (fmode >= 0) {
    const size_t n = (size_t)lo.NS * lo.forced.unit;
    if (f.ids) HIPCK(hipMemcpyAsync(ws + lo.forced, f.ids, n, hipMemcpyDeviceToDevice, st), "decode: forced ids copy");
    else HIPCK(hipMemsetAsync(ws + lo.forced, 0xff, n, st), "decode: forced ids clear");
  }
  if (!graph) {
    Enq q(e, B, o, lo, ws, s, Enq::DECODE);
    q.forced = fmode;
    q.vis_mask = f.vis_mask;
    CK(q.decode_loop());
  } else {
    GraphEntry* hit = nullptr;
    for (auto& g : e->graphs)
      if (g.B == B && g.ws == (void*)ws && g.forced == fmode && memcmp(&g.opts, &o, sizeof(o)) == 0) { hit = &g; break; }
    if (!hit) {
      // capture the loop once: every launch below becomes a kernel node with its arguments frozen (workspace pointers,
      // step index, option values), which is why the key holds all of them
      GraphEntry g;
      g.B = B; g.ws = (void*)ws; g.opts = o; g.forced = fmode; g.graph = nullptr; g.exec = nullptr;
      if (!e->cap) HIPCK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking), "decode: capture stream");
      HIPCK(hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal), "decode: begin capture");
      Enq q(e, B, o, lo, ws, (void*)e->cap, Enq::DECODE);
      q.forced = fmode;
      const int rc = q.decode_loop();
      const hipError_t he = hipStreamEndCapture(e->cap, &g.graph);
      if (rc != VITCAP_OK) { if (g.graph) (void)hipGraphDestroy(g.graph); return rc; }
      HIPCK(he, "decode: end capture");
      HIPCK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0), "decode: graph instantiate");
      if (e->graphs.size() >= 16) drop_graphs(e);        // bounded cache
      e->graphs.push_back(g);
      hit = &e->graphs.back();
    }
    HIPCK(hipGraphLaunch(hit->exec, st), "decode: graph launch");
  }
  const size_t L = (size_t)lo.L;
  if (lo.cbs) {       // [B][1][max_length]: the n_pred words of the selected beam (no BOS column), then pad; tap "cbs_npred" = n_pred
    HIPCK(hipMemcpyAsync(out_ids, ws + lo.cbs_fin_ids, (size_t)B * L * 8, hipMemcpyDeviceToDevice, st), "decode: output copy");
    HIPCK(hipMemcpyAsync(out_logprobs, ws + lo.cbs_fin_lp, (size_t)B * 4, hipMemcpyDeviceToDevice, st), "decode: output copy");
  } else if (lo.beam) {
    const size_t n = (size_t)B * o.num_keep_best;
    HIPCK(hipMemcpyAsync(out_ids, ws + lo.fin_ids, n * L * 8, hipMemcpyDeviceToDevice, st), "decode: output copy");
    HIPCK(hipMemcpyAsync(out_logprobs, ws + lo.fin_lp, n * 4, hipMemcpyDeviceToDevice, st), "decode: output copy");
  } else {
    HIPCK(hipMemcpyAsync(out_ids, ws + lo.ids, (size_t)lo.NS * L * 8, hipMemcpyDeviceToDevice, st), "decode: output copy");
    HIPCK(hipMemcpyAsync(out_logprobs, ws + lo.logprob, (size_t)lo.NS * 4, hipMemcpyDeviceToDevice, st), "decode: output copy");
    // the token chosen at the last position before the forced [SEP] (its log-probability is what the score holds)
    if (out_last_tok)
      HIPCK(hipMemcpyAsync(out_last_tok, ws + lo.last_tok, (size_t)lo.NS * 8, hipMemcpyDeviceToDevice, st), "decode: last-token copy");
    if (f.out_tok_lp)
      HIPCK(hipMemcpyAsync(f.out_tok_lp, ws + lo.tok_lp, (size_t)lo.NS * lo.tok_lp.unit, hipMemcpyDeviceToDevice, st), "decode: token log-probs copy");
  }
  return VITCAP_OK;
}

int tags_copy(const Layout& lo, int B, char* ws, float* tag_logits_out, int64_t* tag_topk_out, void* s) {
  if (tag_logits_out)      // the rows without their padding columns
    HIPCK(hipMemcpy2DAsync(tag_logits_out, (size_t)VITCAP_VOCAB * 4, ws + lo.tag_logits, lo.tag_logits.unit, (size_t)VITCAP_VOCAB * 4, B,
                           hipMemcpyDeviceToDevice, (hipStream_t)s), "tags: logits copy");
  if (tag_topk_out)
    HIPCK(hipMemcpyAsync(tag_topk_out, ws + lo.tag_ids, B * lo.tag_ids.unit, hipMemcpyDeviceToDevice, (hipStream_t)s), "tags: topk copy");
  return VITCAP_OK;
}

}  // namespace

extern "C" void vitcap_gen_opts_init(vitcap_gen_opts* o) {
  if (o) *o = default_opts();
}
extern "C" int vitcap_gen_opts_check(const vitcap_gen_opts* o) {
  if (!o) return VITCAP_OK;
  return check_opts(*o);
}

extern "C" int vitcap_engine_create(vitcap_engine** out) {
  if (!out) return VITCAP_EINVAL;
  *out = new (std::nothrow) vitcap_engine();
  if (*out) {
    const char* t = getenv("VITCAP_FULL_TAG_BLOCK");
    (*out)->full_last_tag_block = t ? atoi(t) != 0 : false;
  }
  return *out ? VITCAP_OK : VITCAP_EINVAL;
}

extern "C" void vitcap_engine_destroy(vitcap_engine* e) {
  if (!e) return;
  for (auto& t : e->pool) {
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
  }
  drop_graphs(e);
  if (e->cap) (void)hipStreamDestroy(e->cap);          // side / dec2 / part streams belong to the process (role_stream)
  for (hipEvent_t ev : {e->ev_fork, e->ev_join, e->ev_dfork, e->ev_djoin, e->ev_pjoin[0], e->ev_pjoin[1], e->ev_pjoin[2], e->ev_pfork})
    if (ev) (void)hipEventDestroy(ev);
  delete e;
}
extern "C" int vitcap_engine_graph_count(vitcap_engine* e) { return e ? (int)e->graphs.size() : 0; }

extern "C" int vitcap_engine_bind_weights(vitcap_engine* e, const vitcap_weights* w) {
  if (!e || !w) { vitcap_set_error("bind_weights: null"); return VITCAP_EINVAL; }
  const void* const* p = (const void* const*)w;
  const size_t required = offsetof(vitcap_weights, xword_emb) / sizeof(void*);      // bert.extra_embeddings is optional
  for (size_t i = 0; i < required; ++i)
    if (!p[i]) { vitcap_set_error("bind_weights: pointer #%zu of vitcap_weights is NULL", i); return VITCAP_EINVAL; }
  std::lock_guard<std::mutex> lk(e->mu);
  e->w = *w;
  e->bound = true;
  drop_graphs(e);          // captured loops hold the old weight pointers
  return VITCAP_OK;
}

extern "C" size_t vitcap_engine_workspace_bytes(int B, const vitcap_gen_opts* opts) {
  const vitcap_gen_opts o = opts_or_default(opts);
  if (B <= 0 || check_opts(o) != VITCAP_OK) return 0;
  return Layout(B, o).off;
}

extern "C" int vitcap_engine_encode(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                    void* workspace, size_t workspace_bytes, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return Enq(e, B, o, lo, (char*)workspace, s, Enq::ENCODE).encode(image, image_is_bf16);
}

extern "C" int vitcap_engine_prefill(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                     void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return Enq(e, B, o, lo, (char*)workspace, s, Enq::ENCODE).prefill();
}

// patch removal: the options a removed patch cannot be honoured under, and the mask pointer, before anything is enqueued
static int check_patches(const char* who, const vitcap_gen_opts& o, const uint32_t* patch_mask) {
  if (!patch_mask) { vitcap_set_error("%s: patch_mask is null", who); return VITCAP_EINVAL; }
  if (((uintptr_t)patch_mask & 3) != 0) { vitcap_set_error("%s: patch_mask is not 4-byte aligned", who); return VITCAP_EINVAL; }
  if (o.tag_visible > 0) { vitcap_set_error("%s: tag_visible > 0 is not supported under patch removal (the tag rows' prefill is unmasked)", who); return VITCAP_EINVAL; }
  if (o.use_graph != 0) { vitcap_set_error("%s: use_graph = 1 is not supported under patch removal (a captured loop would freeze this call's mask)", who); return VITCAP_EINVAL; }
  return VITCAP_OK;
}

extern "C" int vitcap_engine_encode_patches(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                            void* workspace, size_t workspace_bytes, const uint32_t* patch_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(check_patches("encode_patches", o, patch_mask));      // by name, before the workspace these options would size is looked at
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  Enq q(e, B, o, lo, (char*)workspace, s, Enq::ENCODE);
  q.patch_mask = patch_mask;
  return q.encode(image, image_is_bf16);
}

extern "C" int vitcap_engine_prefill_patches(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                             const uint32_t* patch_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(check_patches("prefill_patches", o, patch_mask));      // by name, before the workspace these options would size is looked at
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  Enq q(e, B, o, lo, (char*)workspace, s, Enq::ENCODE);
  q.patch_mask = patch_mask;
  return q.prefill();
}

// Encoder attention written out: vitcap_engine_encode as one part on the caller's stream with the tag branch serial, plus one
// vitcap_attn_self_maps launch behind the attention of every selected block (Enq::emit_block_maps).
extern "C" int vitcap_engine_encode_maps(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                         void* workspace, size_t workspace_bytes, uint32_t block_mask, int per_head, float* maps,
                                         size_t maps_bytes, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  const char* who = "encode_maps";
  if (block_mask == 0 || (block_mask >> 16) != 0) { vitcap_set_error("%s: block_mask must select at least one of bits 0..15 (got 0x%x)", who, block_mask); return VITCAP_EINVAL; }
  if (per_head != 0 && per_head != 1) { vitcap_set_error("%s: per_head must be 0 or 1 (got %d)", who, per_head); return VITCAP_EINVAL; }
  if (!maps) { vitcap_set_error("%s: maps is null", who); return VITCAP_EINVAL; }
  if (((uintptr_t)maps & 3) != 0) { vitcap_set_error("%s: maps is not 4-byte aligned", who); return VITCAP_EINVAL; }
  if (o.use_graph != 0) { vitcap_set_error("%s: use_graph = 1 is not supported (the maps are written by this call's own launches, not by a captured loop)", who); return VITCAP_EINVAL; }
  if (o.tag_visible > 0) { vitcap_set_error("%s: tag_visible > 0 is not supported (the rollout has no path for the tag rows)", who); return VITCAP_EINVAL; }
  if (B > 0) {
    const size_t need = (size_t)__builtin_popcount(block_mask) * B * (per_head ? 12 : 1) * NV * NV * sizeof(float);
    if (maps_bytes < need) { vitcap_set_error("%s: maps_bytes %zu < required %zu bytes", who, maps_bytes, need); return VITCAP_EINVAL; }
  }
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  if (!image) { vitcap_set_error("%s: null image", who); return VITCAP_EINVAL; }
  std::lock_guard<std::mutex> lk(e->mu);
  Enq q(e, B, o, lo, (char*)workspace, s, Enq::ENCODE);
  const Enq::BlockMaps bm{maps, block_mask, per_head};
  q.block_maps = &bm;
  if (e->timing) e->timing_this_step = false;      // timing samples whole steps of the plain calls
  CK(q.encode_part(image, image_is_bf16, false));
  // where vitcap_engine_encode cuts the batch into parts it runs their prefill too (vitcap_engine_prefill then has nothing to do)
  if (q.encode_parts() >= 2) CK(q.prefill_part());
  return VITCAP_OK;
}

extern "C" int vitcap_engine_decode(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                    int64_t* out_ids, float* out_logprobs, int64_t* out_last_tok, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return decode_locked(e, B, o, lo, (char*)workspace, out_ids, out_logprobs, out_last_tok, s);
}

extern "C" int vitcap_engine_decode_forced(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                           const int64_t* forced_ids, int score_forced, int64_t* out_ids, float* out_logprobs,
                                           float* out_token_logprobs, int64_t* out_last_tok, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs;
  CK(check_forced(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return decode_locked(e, B, o, lo, (char*)workspace, out_ids, out_logprobs, out_last_tok, s, f);
}

extern "C" int vitcap_engine_tags(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, float* tag_logits_out,
                                  int64_t* tag_topk_out, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  if (!e || B <= 0 || !workspace || check_opts(o) != VITCAP_OK) { vitcap_set_error("tags: bad arguments"); return VITCAP_EINVAL; }
  return tags_copy(Layout(B, o), B, (char*)workspace, tag_logits_out, tag_topk_out, s);
}

extern "C" int vitcap_engine_generate(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                      void* workspace, size_t workspace_bytes, int64_t* out_ids, float* out_logprobs,
                                      float* tag_logits_out, int64_t* tag_topk_out, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  char* ws = (char*)workspace;
  std::lock_guard<std::mutex> lk(e->mu);
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).encode(image, image_is_bf16));
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).prefill());
  CK(decode_locked(e, B, o, lo, ws, out_ids, out_logprobs, nullptr, s));
  return tags_copy(lo, B, ws, tag_logits_out, tag_topk_out, s);
}

extern "C" int vitcap_engine_generate_forced(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                             void* workspace, size_t workspace_bytes, const int64_t* forced_ids, int score_forced,
                                             int64_t* out_ids, float* out_logprobs, float* out_token_logprobs, float* tag_logits_out,
                                             int64_t* tag_topk_out, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs;
  CK(check_forced(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  char* ws = (char*)workspace;
  std::lock_guard<std::mutex> lk(e->mu);
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).encode(image, image_is_bf16));
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).prefill());
  CK(decode_locked(e, B, o, lo, ws, out_ids, out_logprobs, nullptr, s, f));
  return tags_copy(lo, B, ws, tag_logits_out, tag_topk_out, s);
}

extern "C" int vitcap_engine_decode_masked(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                           const int64_t* forced_ids, int score_forced, int64_t* out_ids, float* out_logprobs,
                                           float* out_token_logprobs, int64_t* out_last_tok, const uint32_t* vis_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs; f.vis_mask = vis_mask; f.masked = true;
  CK(check_masked(o, f));
  CK(check_forced(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return decode_locked(e, B, o, lo, (char*)workspace, out_ids, out_logprobs, out_last_tok, s, f);
}

extern "C" int vitcap_engine_generate_masked(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                             void* workspace, size_t workspace_bytes, const int64_t* forced_ids, int score_forced,
                                             int64_t* out_ids, float* out_logprobs, float* out_token_logprobs, float* tag_logits_out,
                                             int64_t* tag_topk_out, const uint32_t* vis_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs; f.vis_mask = vis_mask; f.masked = true;
  CK(check_masked(o, f));
  CK(check_forced(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  char* ws = (char*)workspace;
  std::lock_guard<std::mutex> lk(e->mu);
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).encode(image, image_is_bf16));
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).prefill());
  CK(decode_locked(e, B, o, lo, ws, out_ids, out_logprobs, nullptr, s, f));
  return tags_copy(lo, B, ws, tag_logits_out, tag_topk_out, s);
}

extern "C" int vitcap_engine_decode_beam_masked(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace,
                                                size_t workspace_bytes, const int64_t* forced_ids, int score_forced, int64_t* out_ids,
                                                float* out_logprobs, float* out_token_logprobs, int64_t* out_last_tok,
                                                const uint32_t* vis_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs; f.vis_mask = vis_mask; f.masked = true;
  CK(check_beam_masked(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  return decode_locked(e, B, o, lo, (char*)workspace, out_ids, out_logprobs, out_last_tok, s, f);
}

extern "C" int vitcap_engine_generate_beam_masked(vitcap_engine* e, const void* image, int image_is_bf16, int B,
                                                  const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                                  const int64_t* forced_ids, int score_forced, int64_t* out_ids, float* out_logprobs,
                                                  float* out_token_logprobs, float* tag_logits_out, int64_t* tag_topk_out,
                                                  const uint32_t* vis_mask, void* s) {
  const vitcap_gen_opts o = opts_or_default(opts);
  Forced f;
  f.ids = forced_ids; f.score = score_forced; f.out_tok_lp = out_token_logprobs; f.vis_mask = vis_mask; f.masked = true;
  CK(check_beam_masked(o, f));
  Layout lo;
  CK(enter(e, B, o, workspace, workspace_bytes, lo));
  char* ws = (char*)workspace;
  std::lock_guard<std::mutex> lk(e->mu);
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).encode(image, image_is_bf16));
  CK(Enq(e, B, o, lo, ws, s, Enq::ENCODE).prefill());
  CK(decode_locked(e, B, o, lo, ws, out_ids, out_logprobs, nullptr, s, f));
  return tags_copy(lo, B, ws, tag_logits_out, tag_topk_out, s);
}

// ---- one-pass scoring of given captions (include/vitcap_hip.h: vitcap_engine_score) ---------------------------------------------
// Every token of a scored caption is known, so the max_length - 1 sequential steps of the forced decode loop become ONE pass over a
// [token rows | [MASK] probe rows] grid per caption: full-size GEMMs on captions x (2L - 1) rows, vitcap_attn_text_grid against
// the image's visual K/V of the prefill, the LM head on the probe rows only (vocabulary GEMM in chunks of SCORE_CHUNK rows) and
// vitcap_score_rows.  Rounding points as step_forward: fp32 residual stream, bf16 GEMM operands, bf16 qkv.
namespace {

// what the one-pass path does not run, refused by name before anything is enqueued
int check_score(const vitcap_gen_opts& o, int caps_per_image) {
#define SC_REQ(cond, ...) do { if (!(cond)) { vitcap_set_error(__VA_ARGS__); return VITCAP_EINVAL; } } while (0)
  SC_REQ(o.num_beams <= 1, "engine_score: num_beams must be 1 (got %d): a caption is scored, not searched", o.num_beams);
  SC_REQ(!o.use_cbs, "engine_score: use_cbs is not run by the one-pass scorer");
  SC_REQ(o.tag_visible <= 0, "engine_score: tag_visible > 0 (got %d) is not built for the one-pass scorer", o.tag_visible);
  SC_REQ(!o.sampling.do_sample, "engine_score: sampling.do_sample is not run by the one-pass scorer (nothing is drawn)");
  SC_REQ(o.repetition_penalty == 1.0f, "engine_score: repetition_penalty must be 1 (got %g): the stepwise path scores the penalised row, "
         "the one-pass path does not build it", (double)o.repetition_penalty);
  SC_REQ(caps_per_image >= 1 && caps_per_image <= SCORE_MAX_CAPS, "engine_score: caps_per_image must be 1..%d (got %d)", SCORE_MAX_CAPS,
         caps_per_image);
#undef SC_REQ
  return check_opts(o);
}

// prefix of the batch refusal, by vitcap_score_req.kind
const char* const SCORE_WHO[4] = {"engine_score", "engine_score_masked", "engine_explain", "engine_alternatives"};

int check_score_io(const vitcap_score_req& r, const ScoreLayout& sl) {
  if (!r.caption_ids || !r.out_logprobs || !r.out_ids) { vitcap_set_error("engine_score: null caption_ids / outputs"); return VITCAP_EINVAL; }
  if (!r.score_ws || ((uintptr_t)r.score_ws & 255) != 0) {
    vitcap_set_error("engine_score: score workspace null or not 256-byte aligned");
    return VITCAP_EINVAL;
  }
  if (r.score_ws_bytes < sl.off) {
    vitcap_set_error("engine_score: score workspace %zu < required %zu bytes", r.score_ws_bytes, sl.off);
    return VITCAP_EWORKSPACE;
  }
  return VITCAP_OK;
}

// VITCAP_SCORE_MAPS: attention maps of the probes, into the caller's [NC][L][4]([12])[W] array; layer_mask bit l: decoder layer l
int check_maps(const vitcap_score_req& r) {
  if (!r.maps) { vitcap_set_error("engine_explain: maps is null"); return VITCAP_EINVAL; }
  if (r.per_head != 0 && r.per_head != 1) { vitcap_set_error("engine_explain: per_head must be 0 or 1 (got %d)", r.per_head); return VITCAP_EINVAL; }
  if (r.layer_mask < 1 || r.layer_mask > 15) {
    vitcap_set_error("engine_explain: layer_mask must select at least one of the 4 decoder layers (1..15, got %d)", r.layer_mask);
    return VITCAP_EINVAL;
  }
  return VITCAP_OK;
}

// VITCAP_SCORE_ALTS: token alternatives of the probe rows, into the caller's alt_ids / alt_lp [NC][L][k] and rank / entropy [NC][L]
int check_alts(const vitcap_score_req& r) {
  if (r.k < 1 || r.k > 16) { vitcap_set_error("engine_alternatives: k must be 1..16 (got %d)", r.k); return VITCAP_EINVAL; }
  if (!r.alt_ids || !r.alt_lp || !r.rank || !r.entropy) {
    vitcap_set_error("engine_alternatives: null alt_ids / alt_lp / rank / entropy");
    return VITCAP_EINVAL;
  }
  return VITCAP_OK;
}

// reads lo.dqkv[0..3] of the workspace (the visual caches of the prefill) and nothing else of it.  VITCAP_SCORE_MASKED: vis_mask
// [NC][19] (vitcap_attn_text_grid_masked's layout) is the caller's array, read in place by the attention launches of all four layers.
int score_locked(vitcap_engine* e, const vitcap_score_req& r, const vitcap_gen_opts& o, const Layout& lo, const ScoreLayout& sl, void* s) {
  hipStream_t st = (hipStream_t)s;
  const int B = r.B, L = sl.L, R = sl.R, K = sl.K;
  const int NC = (int)sl.NC, M = (int)sl.M, P = (int)sl.P;
  const bool masked = r.kind == VITCAP_SCORE_MASKED, maps = r.kind == VITCAP_SCORE_MAPS, alts = r.kind == VITCAP_SCORE_ALTS;
  char* ws = (char*)r.workspace;
  char* sw = (char*)r.score_ws;
  Enq q(e, B, o, lo, ws, s, Enq::ENCODE);
  const vitcap_weights& w = e->w;
  int64_t* ids = sl.ids.at<int64_t>(sw);
  int64_t* last = sl.last_tok.at<int64_t>(sw);
  HIPCK(hipMemcpyAsync(ids, r.caption_ids, (size_t)NC * L * 8, hipMemcpyDeviceToDevice, st), "engine_score: caption ids copy");
  if (r.last_tok) HIPCK(hipMemcpyAsync(last, r.last_tok, (size_t)NC * 8, hipMemcpyDeviceToDevice, st), "engine_score: last_tok copy");
  else HIPCK(hipMemsetAsync(last, 0xff, (size_t)NC * 8, st), "engine_score: last_tok clear");
  float* x_f = sl.x_f.at<float>(sw);
  char* x_b = sw + sl.x_b;
  CK(vc_score_grid_ids(ids, sl.grid_ids.at<int64_t>(sw), NC, L, o.mask_token_id, o.pad_token_id, s));
  CK(vitcap_embed_rows(sl.grid_ids.at<int64_t>(sw), R, w.word_emb, w.pos_emb, w.type_emb, w.emb_ln_g, w.emb_ln_b, 1e-12f, nullptr, x_f, x_b,
                       M, L, s));
  for (int l = 0; l < 4; ++l) {
    const vitcap_bert_layer_w& lw = w.dec[l];
    const char* vis = ws + lo.dqkv[l];
    CK(q.gemm(x_b, D, lw.qkv_w, lw.qkv_b, nullptr, 0, sw + sl.qkv, 3 * D, M, 3 * D, D, VITCAP_ACT_NONE, VITCAP_OUT_BF16));
    if (maps && ((r.layer_mask >> l) & 1))      // the caller's array, this layer's slice; reads qkv and the ids only
      CK(vitcap_attn_probe_maps(sw + sl.qkv, vis, ids, r.maps + (size_t)l * (r.per_head ? 12 : 1) * (SV + L), B, K, SV, L, r.per_head,
                                o.eos_token_id, o.eos_extra, 0.125f, s));
    CK(vitcap_attn_beam_vt(vis, sw + sl.vt, B, SV, s));
    if (masked) CK(vitcap_attn_text_grid_masked(sw + sl.qkv, vis, sw + sl.vt, r.vis_mask, sw + sl.ctx, B, K, SV, L, 0.125f, s));
    else CK(vitcap_attn_text_grid(sw + sl.qkv, vis, sw + sl.vt, sw + sl.ctx, B, K, SV, L, 0.125f, s));
    // BertSelfOutput / BertIntermediate / BertOutput: dense + residual, then LayerNorm (post-LN), as prefill_part
    CK(q.gemm_ln(sw + sl.ctx, D, lw.ao_w, lw.ao_b, x_f, sw + sl.tmp, M, D, lw.ao_g, lw.ao_beta, 1e-12f, sw + sl.sa_b, sl.sa_f.at<float>(sw)));
    CK(q.gemm(sw + sl.sa_b, D, lw.i_w, lw.i_b, nullptr, 0, sw + sl.mlp, 4 * D, M, 4 * D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_BF16));
    CK(q.gemm_ln(sw + sl.mlp, 4 * D, lw.o_w, lw.o_b, sl.sa_f.at<float>(sw), sw + sl.tmp, M, 4 * D, lw.o_g, lw.o_beta, 1e-12f, x_b, x_f));
  }
  // LM head on the probe rows (rows L .. 2L-2 of every caption): transform (dense + GELU + LayerNorm), then the vocabulary GEMM in chunks
  CK(vitcap_copy_row_blocks(x_b, R, L, D, 0, sw + sl.hd_in, L - 1, 0, D, 0, L - 1, D, NC, s));
  CK(q.gemm(sw + sl.hd_in, D, w.cls.dense_w, w.cls.dense_b, nullptr, 0, sw + sl.hd_f, D, P, D, D, VITCAP_ACT_GELU_ERF, VITCAP_OUT_F32));
  CK(vitcap_layernorm_fwd(sl.hd_f.at<float>(sw), D, w.cls.ln_g, w.cls.ln_b, 1e-12f, sw + sl.hd_b, nullptr, P, D, s));
  float* tok_lp = r.out_token_logprobs ? r.out_token_logprobs : sl.tok_lp.at<float>(sw);
  if (alts) {      // the dead pattern once: column 0 and whatever no launch covers; the chunks' launches write the rest
    const size_t n = (size_t)NC * L;
    HIPCK(hipMemsetAsync(r.alt_ids, 0xff, n * r.k * 4, st), "engine_alternatives: alt_ids clear");
    HIPCK(hipMemsetAsync(r.rank, 0xff, n * 4, st), "engine_alternatives: rank clear");
    HIPCK(hipMemsetAsync(r.alt_lp, 0, n * r.k * 4, st), "engine_alternatives: alt_lp clear");
    HIPCK(hipMemsetAsync(r.entropy, 0, n * 4, st), "engine_alternatives: entropy clear");
  }
  for (int r0 = 0; r0 < P; r0 += (int)sl.CH) {
    const int n = P - r0 < (int)sl.CH ? P - r0 : (int)sl.CH;
    CK(q.gemm(sl.hd_b.at<char>(sw, (size_t)r0), D, w.cls.dec_w, w.cls.dec_b, nullptr, 0, sw + sl.logits, VP, n, VP, D, VITCAP_ACT_NONE,
              VITCAP_OUT_F32));
    if (alts)      // one kernel does vitcap_score_rows' job too: the 250 MB chunk is read once
      CK(vc_score_rows_alts(sl.logits.at<float>(sw), VP, VITCAP_VOCAB, ids, last, r0, n, NC, L, o.eos_token_id, o.eos_extra, o.pad_token_id,
                            tok_lp, r.out_ids, r.out_last_tok, r.out_logprobs, r.k, r.alt_ids, r.alt_lp, r.rank, r.entropy, s));
    else
      CK(vitcap_score_rows(sl.logits.at<float>(sw), VP, VITCAP_VOCAB, ids, last, r0, n, NC, L, o.eos_token_id, o.eos_extra, o.pad_token_id,
                           nullptr, nullptr, tok_lp, r.out_ids, r.out_last_tok, r.out_logprobs, s));
  }
  return VITCAP_OK;
}

// Every one-pass request, every refusal in one order: the request itself (null, ABI, kind), options, batch, the kind's own fields
// (mask / maps / alternatives), io, workspace -- then, with `encode`, encode + prefill, then score_locked.
int score_entry(vitcap_engine* e, const vitcap_score_req* rp, void* s) {
  if (!rp) { vitcap_set_error("score_req: null request"); return VITCAP_EINVAL; }
  const vitcap_score_req& r = *rp;
  if (r.abi != VITCAP_ABI_VERSION) {
    vitcap_set_error("score_req: built against ABI %d, this library is ABI %d (use vitcap_score_req_init)", r.abi, VITCAP_ABI_VERSION);
    return VITCAP_EINVAL;
  }
  if (r.kind < VITCAP_SCORE_PLAIN || r.kind > VITCAP_SCORE_ALTS) {
    vitcap_set_error("score_req: kind must be one of VITCAP_SCORE_* (0..3, got %d)", r.kind);
    return VITCAP_EINVAL;
  }
  const vitcap_gen_opts o = opts_or_default(r.opts);
  CK(check_score(o, r.caps_per_image));
  if (r.B <= 0) { vitcap_set_error("%s: bad batch", SCORE_WHO[r.kind]); return VITCAP_EINVAL; }
  if (r.kind == VITCAP_SCORE_MASKED) {
    if (!r.vis_mask) { vitcap_set_error("engine_score_masked: vis_mask is null"); return VITCAP_EINVAL; }
    if (((uintptr_t)r.vis_mask & 3) != 0) { vitcap_set_error("engine_score_masked: vis_mask is not 4-byte aligned"); return VITCAP_EINVAL; }
  }
  if (r.kind == VITCAP_SCORE_MAPS) CK(check_maps(r));
  if (r.kind == VITCAP_SCORE_ALTS) CK(check_alts(r));
  const ScoreLayout sl(r.B, r.caps_per_image, o.max_length);
  CK(check_score_io(r, sl));
  Layout lo;
  CK(enter(e, r.B, o, r.workspace, r.workspace_bytes, lo));
  std::lock_guard<std::mutex> lk(e->mu);
  if (r.encode) {
    char* ws = (char*)r.workspace;
    CK(Enq(e, r.B, o, lo, ws, s, Enq::ENCODE).encode(r.image, r.image_is_bf16));
    CK(Enq(e, r.B, o, lo, ws, s, Enq::ENCODE).prefill());
  }
  return score_locked(e, r, o, lo, sl, s);
}

}  // namespace

extern "C" size_t vitcap_engine_score_workspace_bytes(int B, int caps_per_image, const vitcap_gen_opts* opts) {
  const vitcap_gen_opts o = opts_or_default(opts);
  if (B <= 0 || check_score(o, caps_per_image) != VITCAP_OK) return 0;
  return ScoreLayout(B, caps_per_image, o.max_length).off;
}

extern "C" void vitcap_score_req_init(vitcap_score_req* r) {
  if (!r) return;
  *r = vitcap_score_req();
  r->abi = VITCAP_ABI_VERSION;
  r->kind = VITCAP_SCORE_PLAIN;
}

extern "C" int vitcap_engine_score_req(vitcap_engine* e, const vitcap_score_req* r, void* s) { return score_entry(e, r, s); }

// The plain request with positional arguments in place of the struct, as every integration starts.
namespace {
vitcap_score_req plain_req(int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes, int caps_per_image,
                           const int64_t* caption_ids, const int64_t* last_tok, void* score_ws, size_t score_ws_bytes,
                           float* out_logprobs, float* out_token_logprobs, int64_t* out_ids, int64_t* out_last_tok) {
  vitcap_score_req r;
  vitcap_score_req_init(&r);
  r.B = B; r.opts = opts; r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.caps_per_image = caps_per_image; r.caption_ids = caption_ids; r.last_tok = last_tok;
  r.score_ws = score_ws; r.score_ws_bytes = score_ws_bytes;
  r.out_logprobs = out_logprobs; r.out_token_logprobs = out_token_logprobs; r.out_ids = out_ids; r.out_last_tok = out_last_tok;
  return r;
}
}  // namespace

extern "C" int vitcap_engine_score_text(vitcap_engine* e, int B, const vitcap_gen_opts* opts, void* workspace, size_t workspace_bytes,
                                        int caps_per_image, const int64_t* caption_ids, const int64_t* last_tok, void* score_ws,
                                        size_t score_ws_bytes, float* out_logprobs, float* out_token_logprobs, int64_t* out_ids,
                                        int64_t* out_last_tok, void* s) {
  const vitcap_score_req r = plain_req(B, opts, workspace, workspace_bytes, caps_per_image, caption_ids, last_tok, score_ws, score_ws_bytes,
                                       out_logprobs, out_token_logprobs, out_ids, out_last_tok);
  return score_entry(e, &r, s);
}

extern "C" int vitcap_engine_score(vitcap_engine* e, const void* image, int image_is_bf16, int B, const vitcap_gen_opts* opts,
                                   void* workspace, size_t workspace_bytes, int caps_per_image, const int64_t* caption_ids,
                                   const int64_t* last_tok, void* score_ws, size_t score_ws_bytes, float* out_logprobs,
                                   float* out_token_logprobs, int64_t* out_ids, int64_t* out_last_tok, void* s) {
  vitcap_score_req r = plain_req(B, opts, workspace, workspace_bytes, caps_per_image, caption_ids, last_tok, score_ws, score_ws_bytes,
                                 out_logprobs, out_token_logprobs, out_ids, out_last_tok);
  r.encode = 1; r.image = image; r.image_is_bf16 = image_is_bf16;
  return score_entry(e, &r, s);
}

extern "C" const void* vitcap_engine_tap(vitcap_engine* e, const char* name, void* workspace, int B, const vitcap_gen_opts* opts) {
  const vitcap_gen_opts o = opts_or_default(opts);
  if (!e || !name || !workspace || B <= 0 || check_opts(o) != VITCAP_OK) return nullptr;
  const Layout lo(B, o);
  char* ws = (char*)workspace;
  if (!strcmp(name, "last_token")) return ws + lo.last_tok;
  if (!strcmp(name, "hidden")) return ws + lo.x2;
  if (!strcmp(name, "tag_hidden")) return ws + lo.xt;
  if (!strcmp(name, "vis")) return ws + lo.vis_f;
  if (!strcmp(name, "logits_last")) return ws + lo.logits;
  if (!strcmp(name, "margins")) return ws + lo.margins;
  if (!strcmp(name, "tag_logits")) return ws + lo.tag_logits;
  if (!strcmp(name, "tag_prob")) return ws + lo.tag_prob;
  if (!strcmp(name, "tag_len")) return ws + lo.tag_len;
  if (!strcmp(name, "ids")) return ws + lo.ids;
  if (!strcmp(name, "live")) return ws + lo.live;
  if (!strcmp(name, "cbs_npred")) return lo.cbs ? ws + lo.cbs_npred : nullptr;
  if (!strncmp(name, "dqkv", 4) && name[4] >= '0' && name[4] <= '3' && !name[5]) return ws + lo.dqkv[name[4] - '0'];
  return nullptr;
}
