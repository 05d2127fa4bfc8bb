// Per-call state that the engine hands to the public launchers through thread-locals (defined in error.cpp).  Host-safe: included
// by common.h (every .hip file) and by the engine.  The launchers keep reading these because tests call them directly, with the defaults.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

void vitcap_set_error(const char* fmt, ...);
// argument check of an entry point: record the message, return VITCAP_EINVAL (include/vitcap_hip.h)
#define VC_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) {                            \
      vitcap_set_error(__VA_ARGS__);          \
      return VITCAP_EINVAL;                   \
    }                                         \
  } while (0)

// While vitcap_engine_decode enqueues its step loop, this pointer names the device counter of sequences (beam search: images) still
// unfinished; the decode-step launchers pass it to their kernels, which return at entry once it reads 0 -- the reference's
// `if cur_unfinished.max() == 0: break` (modeling_utils.py:866 / `if all(done): break`, :1072) without a host synchronisation.
// NULL outside the engine.
extern thread_local const int32_t* vc_tls_live;
// Further EOS token ids of the call being enqueued (vitcap_gen_opts.eos_extra; -1 = unused).  The reference's greedy / sampling loop
// stops a sequence at ANY id of `eos_token_ids` (modeling_utils.py:862-865) and forces eos_token_ids[0] at the last position
// (:870-871); the step launchers read this next to their `eos` argument, which stays the first id.
struct VcEosExtra { int32_t id[3]; };
extern thread_local VcEosExtra vc_tls_eos_extra;
// Walk direction of the streaming kernels of the call being enqueued (round 5).  Every kernel of the encoder / prefill chain is one
// pass over the batch's rows; a consumer that walks them in the SAME order as its producer finds, in the 256 MB Infinity Cache, the
// END of what the producer wrote while it asks for the BEGINNING (fc2's A operand at B = 64 is 227 MB: the probe with that operand
// cache-resident runs the kernel 21 % faster, profiles/r05_g4w_probe.txt).  With the flag set a kernel visits its row blocks
// last-to-first, so that what was written last is read first; the engine flips it after every streaming launch.  Results do not
// depend on it (the order in which independent tiles run).  False outside the engine.
extern thread_local bool vc_tls_walk_rev;
extern thread_local bool vc_tls_zigzag;        // the engine call being enqueued alternates directions (GEMM + LayerNorm pairs flip in between)
// Dropout salt (vitcap_set_dropout_salt): a device-resident 32-bit word XORed into every dropout seed by the training kernels.  The
// seeds themselves are launch arguments -- frozen when a training step is captured into a hipGraph -- so a captured step changes its
// keep decisions from replay to replay by rewriting this word (vitcap_amd/train.py, graph mode).  NULL = no salt (the default).
extern thread_local const uint32_t* vc_tls_drop_salt;
// Timing runs only (vitcap_engine_timing_begin): when set, the large-GEMM launchers hand these two events to hipExtLaunchKernelGGL,
// which binds them to THE KERNEL DISPATCH (start = the kernel begins executing, stop = it has completed: the timestamps rocprofv3
// --kernel-trace reports), instead of bracketing the launch with stream markers whose interval also holds the time the dispatch
// waited for the chip behind another stream's kernels.  vc_tls_kev_used tells the engine that a launcher took them.
extern thread_local hipEvent_t vc_tls_kev_start, vc_tls_kev_stop;
extern thread_local bool vc_tls_kev_used;
