// The engine object, shared by engine.cpp (enqueue) and engine_timing.cpp (per-launch GEMM timing).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/vitcap_hip.h"
#include "call_state.h"

// Optional per-launch timing of the large-tile GEMM launches (bench.py's live roofline measurement):
// hipEvents are recorded on the SAME stream right before/after each launch; the pool is grown outside
// the timed region by vitcap_engine_timing_begin().
struct GemmTiming {
  hipEvent_t start, stop;     // stream markers right before / after the launch
  hipEvent_t kstart, kstop;   // bound to the kernel dispatch itself (hipExtLaunchKernelGGL): what rocprofv3 --kernel-trace reports
  bool kernel_bound;          // the launcher took kstart / kstop
  int variant;      // act*4 + out_f32*2 + has_res
  double flops;
};

struct GraphEntry {
  int B;
  void* ws;
  vitcap_gen_opts opts;
  int forced;         // Enq::forced of the captured loop: -1 plain, else score_forced (the staged ids themselves live in the workspace)
  hipGraph_t graph;
  hipGraphExec_t exec;
};

struct vitcap_engine {
  vitcap_weights w;
  bool bound = false;
  bool timing = false;
  int timing_stride = 1;      // the large-GEMM launches of every timing_stride-th STEP (encode call) are timed (vitcap_engine_timing_sample)
  long long timing_seen = 0;  // steps since timing_begin
  bool timing_this_step = true;
  // one enqueue at a time per engine: the side stream / fork-join events and the graph cache are shared by all callers
  std::mutex mu;
  // the tag branch of the encoder (4 tag blocks + tag head) runs on this side stream next to caption blocks 8-11
  hipStream_t side = nullptr;
  hipStream_t cap = nullptr;          // the decode loop is CAPTURED on this engine-owned stream (capture executes nothing), so the
                                      // caller's stream may be any stream, the legacy default stream included
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t dec2 = nullptr;         // second stream of the split decode loop (vitcap_gen_opts.decode_streams = 2)
  hipEvent_t ev_dfork = nullptr, ev_djoin = nullptr;
  hipStream_t part[3] = {nullptr, nullptr, nullptr};   // streams of encoder parts 1..3 (part 0 runs on the caller's stream)
  hipEvent_t ev_pfork = nullptr, ev_pjoin[3] = {nullptr, nullptr, nullptr};   // the parts share one fork event
  bool full_last_tag_block = false;   // VITCAP_FULL_TAG_BLOCK=1: compute all 577 rows of tag_blocks[3] (parity taps / measurements)
  std::vector<GemmTiming> pool;
  size_t used = 0;
  std::vector<GraphEntry> graphs;     // captured decode loops (vitcap_gen_opts.use_graph)
};

// decode.hip: the token ids of the one-pass scorer's text grid, [n_caps][2L-1] = the caption's L tokens (an id outside the vocabulary
// is embedded as `pad`), then L-1 [MASK].  Internal to the engine (vitcap_engine_score*).
int vc_score_grid_ids(const int64_t* ids, int64_t* grid, int n_caps, int L, int mask, int pad, void* stream);
// alternatives.hip: vitcap_score_rows_alts, and with token_logprobs != null vitcap_score_rows' results for the same rows from the same
// read of the chunk (out_ids and logprob_out are then required; bit-identical to vitcap_score_rows).
int vc_score_rows_alts(const float* logits, int ldl, int V, const int64_t* caption_ids, const int64_t* last_tok, int rows0, int n_rows,
                       int n_caps, int max_len, int eos, const int32_t* eos_extra, int pad, float* token_logprobs, int64_t* out_ids,
                       int64_t* out_last_tok, float* logprob_out, int k, int32_t* alt_ids, float* alt_lp, int32_t* rank, float* entropy,
                       void* stream);
