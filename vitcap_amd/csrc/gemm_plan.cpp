// Host only: which kernel runs an NT GEMM (vc_gemm_plan) and the host-side queries that answer from the same functions.  No launch
// happens here; gemm.hip and gemm4w.hip take what the plan says.
#include "gemm_plan.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "call_state.h"

namespace {

int device_cus() {
  static const int n = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      return prop.multiProcessorCount;
    return 256;
  }();
  return n;
}
// workgroups of the persistent grid = CUs it occupies (512 registers per lane: one workgroup owns a CU), less the CUs (a multiple of
// 8: the XCDs stay balanced) that vitcap_gemm_reserve_cus leaves to whatever else runs on the GPU while a collective is in flight
std::atomic<int> g_reserve_cus{0};
int persistent_cus() {
  const int n = device_cus() - g_reserve_cus.load(std::memory_order_relaxed);
  return n >= 8 ? n : 8;
}

// width (in 256-column tiles) of the column groups the 256x256 kernels walk
int tile_group_n(int tiles_n) {
  // measured at M = 36928 (column-group width swept 1..6): N = 3072 214 -> 199 us with groups of 2..6 tiles (W = 4.7 MB does not fit
  // one XCD's 4 MB L2 next to the A tiles; HBM fetch 169 -> 152 MiB per launch); N = 2304 (W = 3.5 MB fits) same time with
  // 7 % MORE fetch when grouped, so only wider outputs are grouped
  return tiles_n > 9 ? 3 : tiles_n;
}

// ---- tile plan of an 8-wave launch: how many rows go to 256-row tiles, and the height of the tiles behind them ------------------
// A launch of T equal tiles on C CUs costs ceil(T / C) tile times: 435 tiles (M = 36928, N = 768) pay 2 rounds for 1.7 rounds of
// work, 1305 (N = 2304) pay 6 for 5.1.  The plan keeps 256-row tiles for the rows that fill whole rounds and cuts the rest into
// 192- or 128-row tiles, chosen by simulating the dispatch (earliest free CU takes the next workgroup) with tile costs relative
// to the 256-row tile (a shorter tile has the same W traffic and per-phase overheads for fewer flops: measured, tools/gemm_bench.py).
struct TilePlan { int tm_big, mts, tm_small; };
TilePlan plan_tiles(int M, int tiles_n, int K) {
  const int n_cu = device_cus();
  const int tm_full = (M + 255) / 256;
  TilePlan best{tm_full, 0, 0};
  struct Key { int M, tn, K; };
  static std::mutex mu;
  static std::vector<std::pair<Key, TilePlan>> cache;
  {
    std::lock_guard<std::mutex> g(mu);
    for (const auto& e : cache)
      if (e.first.M == M && e.first.tn == tiles_n && e.first.K == K) return e.second;
  }
  // relative tile costs: main loop ~ (64 MT + overhead) cycles per phase, epilogue ~ MT; K = 768 tiles are about half epilogue
  const float c3 = 0.80f, c2 = 0.60f;
  float best_t = ceilf((float)(tm_full * tiles_n) / n_cu);
  const float need = best_t * 0.97f;                         // a plan must win 3 % to replace the plain grid
  const int span = (int)(2.5f * n_cu / tiles_n) + 2;         // rows worth ~2.5 rounds can move to short tiles
  std::vector<float> heap;
  for (int mts = 3; mts >= 2; --mts) {
    const float cs = mts == 3 ? c3 : c2;
    for (int tb = tm_full - 1; tb >= 0 && tb >= tm_full - span; --tb) {
      const int rows_left = M - tb * 256;
      const int ts = (rows_left + 64 * mts - 1) / (64 * mts);
      const int nb = tb * tiles_n, ns = ts * tiles_n;
      // big tiles: CU j is free at (nb / C + (j < nb % C)); the short tiles go to the earliest free CU
      heap.assign(n_cu, 0.f);
      for (int j = 0; j < n_cu; ++j) heap[j] = -(float)(nb / n_cu + (j < nb % n_cu ? 1 : 0));
      std::make_heap(heap.begin(), heap.end());              // max-heap of negated free times
      float end = nb ? (float)((nb + n_cu - 1) / n_cu) : 0.f;
      for (int i = 0; i < ns; ++i) {
        std::pop_heap(heap.begin(), heap.end());
        const float f = -heap.back() + cs;
        heap.back() = -f;
        std::push_heap(heap.begin(), heap.end());
        end = f > end ? f : end;
      }
      if (end < need && end < best_t - 1e-4f) { best_t = end; best = TilePlan{tb, mts, ts}; }
    }
  }
  std::lock_guard<std::mutex> g(mu);
  cache.push_back({Key{M, tiles_n, K}, best});
  return best;
}

// ---- the 4-wave kernel's own choices (gemm4w.hip) ---------------------------------------------------------------------------------
// Tile height by launch: a launch of T equal tiles on C CUs costs ceil(T / C) tile times, and a (32 * MI)-row tile costs about
// (fixed + MI) units -- 435 tiles of 256 rows (M = 36928, N = 768) pay 2 rounds for 1.7 rounds of work, 495 tiles of 224 rows pay
// 2 rounds of 7/8 the length; 1305 (N = 2304) pay 6, 1485 of 224 rows pay 6 x 7/8.  The kernel is the same code for every MI (the
// wave tile is MI x 8 MFMA tiles, k order per output element unchanged: bit-identical results whatever the height).
int pick_mi(int M, int tiles_n, int form) {
  const int n_cu = form == 2 ? persistent_cus() : device_cus();
  const float fixed = form == 2 ? 0.3f : 0.9f;       // per-tile cost that does not shrink with the tile: pipeline fill, barriers' skew, W traffic
  int best = 8;
  float best_c = 1e30f;
  for (int mi = 8; mi >= 6; --mi) {
    const long long tiles = (long long)((M + 32 * mi - 1) / (32 * mi)) * tiles_n;
    const float c = (float)((tiles + n_cu - 1) / n_cu) * (fixed + (float)mi);
    if (c < best_c * 0.985f) { best_c = c; best = mi; }      // a shorter tile must win 1.5 % to be taken
  }
  return best;
}

// The form a 4-wave launch really takes (0 = one tile per workgroup + LDS epilogue, 1 = one tile per workgroup + register epilogue,
// 2 = persistent) when `form` was asked for, and its tile height
struct Form4w { int form, mi; };
Form4w form_4w(int form, int M, int N, int K, int ldc, int row_group, bool out_f32, bool res) {
  // the register epilogue's bf16 stores are 16 bytes wide
  const bool regs_ok = out_f32 || res || ((N & 7) == 0 && (ldc & 7) == 0);
  if (form != 0 && !regs_ok) form = 0;
  // the persistent pipeline's tile body needs three k-tiles; its epilogues address plain rows of whole 256-column tiles
  if (form == 2 && (K < 192 || (N & 255) != 0 || row_group != 0 || (!out_f32 && (ldc & 7) != 0))) form = 1;
  return Form4w{form, form == 0 ? 8 : pick_mi(M, (N + 255) / 256, form)};
}

constexpr int BUF_4W = 2 * 256 * 128;                                                    // gemm4w.hip: A k-tile + W k-tile
constexpr int SMEM_4W = 4 * 128 * 272 > 2 * BUF_4W ? 4 * 128 * 272 : 2 * BUF_4W;         // LDS epilogue: four 128 x 64 fp32 patches
constexpr int SMEM_4WP = 2 * BUF_4W + 4 * 16 * 512;                                      // register epilogue, fp32 path: = 160 KiB

bool supports_4w(const vitcap_gemm_desc* d, const GemmOperands& o, int split_k) {
  const int act = d->act;
  if (o.aux || o.zout || d->colsum) {
    // training extras: the PERSISTENT form's bf16 register epilogue only (form_4w never downgrades under these conditions: the caller
    // checks that the persistent form was chosen) -- plain rows, whole 256-column tiles, 16-byte aligned rows of every operand
    return !o.res && !d->rowstat && !d->live && split_k <= 1 && d->K >= 192 && (d->N & 255) == 0 && d->row_group == 0 && (d->ldc & 7) == 0 &&
           (!o.aux || (o.ldaux & 7) == 0) && (!o.zout || (o.ldz & 7) == 0) && d->M >= 2048 &&
           (act == VITCAP_ACT_NONE || act == VITCAP_ACT_GELU_ERF);
  }
  // d->live (decode loops: early exit once every sequence has finished) is honoured by the 8-wave kernels only: such launches stay there
  return !d->rowstat && !d->live && split_k <= 1 && d->K >= 128 && (act == VITCAP_ACT_NONE || act == VITCAP_ACT_GELU_ERF);
}

int plan_4w(const vitcap_gemm_desc* d, const GemmOperands& o, int split_k, int form, GemmPlan* pl) {
  VC_REQUIRE(supports_4w(d, o, split_k), "gemm(4-wave): unsupported options (training extras / split-K / activation %d / K < 128)", d->act);
  const bool out_f32 = d->out_dtype == VITCAP_OUT_F32;
  VC_REQUIRE(out_f32 || d->out_dtype == VITCAP_OUT_BF16, "gemm(4-wave): unsupported act %d / out %d", d->act, d->out_dtype);
  const Form4w f = form_4w(form, d->M, d->N, d->K, d->ldc, d->row_group, out_f32, o.res);
  pl->family = f.form == 2 ? VITCAP_GEMM_FAMILY_4WAVE_PERSISTENT : VITCAP_GEMM_FAMILY_4WAVE_TILE;
  pl->act = d->act; pl->out_f32 = out_f32; pl->has_res = o.res;
  pl->form = f.form; pl->mi = f.mi;
  pl->tiles_n = (d->N + 255) / 256;
  pl->group_n = tile_group_n(pl->tiles_n);
  pl->tiles_m = (d->M + 32 * f.mi - 1) / (32 * f.mi);
  pl->n_big = pl->tiles_m * pl->tiles_n;
  pl->grid[0] = pl->n_big;
  pl->lds_bytes = f.form == 0 ? SMEM_4W : (out_f32 || o.res) ? SMEM_4WP : 2 * BUF_4W;
  if (f.form != 2) return VITCAP_OK;
  const int n_cu = persistent_cus();
  pl->grid[0] = pl->n_big < n_cu ? pl->n_big : n_cu;
  if (out_f32 || o.res) return VITCAP_OK;
  if (o.aux || o.zout || d->colsum) {        // training extras: the bf16 register epilogue's second form (supports_4w)
    pl->variant = VITCAP_GEMM_4W_EXTRAS;
    return VITCAP_OK;
  }
  // deferred stores (round 6): the upper half of every wave tile's stores ride behind the next tile's first k-tiles.  Measured
  // (profiles/r06_deferred_stores.txt): the epilogue shrinks as priced (qkv 8.7k -> 6.2k cycles per tile), but with ONE wave per
  // SIMD a store's issue (~150 cycles each) stalls the wave wherever it stands, so the next tile's loop pays what the epilogue
  // saved (25.3k -> 27.2k + 0.7k): a tie without an activation (qkv 138.9 -> 138.3 us, the training step 49.63 -> 49.23 ms),
  // a loss with GELU (fc1 211.8 -> 221.0 us: its stores were already hidden behind the activation's arithmetic) and from 64k rows
  // on, where the parked stores compete with the A panel's HBM stream (qkv 1 080 -> 1 153 us; B = 512 pipeline 4 160 -> 4 064
  // img/s).  Policy: plain bf16 outputs below 64k rows.  VITCAP_GEMM_4W_DEFER: 0 = never, 1 = that policy (default), 2 = always.
  const char* de = getenv("VITCAP_GEMM_4W_DEFER");      // read per plan (not cached): the parity test switches it
  const int defer = de ? atoi(de) : 1;
  const bool want = defer == 2 || (defer == 1 && d->act == VITCAP_ACT_NONE && d->M < 65536);
  if (want && d->K / 64 >= f.mi / 2 + 3) {              // the parked m-tiles (gemm4w.hip: Park<MI>::NP = MI / 2) each ride one k-tile
    pl->variant = VITCAP_GEMM_4W_DEFER;
    return VITCAP_OK;
  }
  // A-panel prefetch one tile ahead (round 5's measured probe, shipped in round 6): from ~64k rows on the A panel streams from
  // HBM and the same loop takes 32-37k instead of 25.4k cycles per tile; whole rows of the NEXT tile's panel, split over the column
  // siblings, requested one per k-tile bring it to 29.7k (qkv +3.6 %, fc1 +2.1 % wall at M = 295 424, docs/LAB_r05.md section 1).
  // Below the threshold the operands are cache-resident and the extra instruction only costs (+0.8 % loop cycles): plain form.
  if (f.mi == 8 && d->M >= 65536 && pl->tiles_m > 1) {
    pl->variant = VITCAP_GEMM_4W_PREFETCH;
    pl->lds_bytes = 2 * BUF_4W + 1024;
  }
  return VITCAP_OK;
}

// 8-wave 256x256 kernel.  mix: -1 = plan_tiles decides, 0 = 256-row tiles only, 3 / 2 = every tile 192 / 128 rows (tile-cost measurements)
int plan_8w(const vitcap_gemm_desc* d, const GemmOperands& o, int mix, GemmPlan* pl) {
  VC_REQUIRE((d->act == VITCAP_ACT_NONE || d->act == VITCAP_ACT_GELU_ERF) && (d->out_dtype == VITCAP_OUT_BF16 || d->out_dtype == VITCAP_OUT_F32),
             "gemm(256): unsupported act %d / out %d", d->act, d->out_dtype);
  const bool extras = o.aux || o.zout || d->colsum;     // training extras (PH | 8 build) and fused-LayerNorm launches: 256-row tiles only
  pl->family = VITCAP_GEMM_FAMILY_8WAVE;
  pl->act = d->act; pl->out_f32 = d->out_dtype; pl->has_res = o.res;
  pl->ph = pl->ln_fused ? (4 | 512) : extras ? (4 | 8) : 4;
  pl->tiles_n = (d->N + 255) / 256;
  pl->group_n = tile_group_n(pl->tiles_n);
  TilePlan t{(d->M + 255) / 256, 0, 0};
  if (extras || pl->ln_fused) mix = 0;
  if (mix < 0) t = plan_tiles(d->M, pl->tiles_n, d->K);
  else if (mix > 0) t = TilePlan{0, mix, (d->M + 64 * mix - 1) / (64 * mix)};
  pl->mts = t.mts;
  pl->tiles_m = t.tm_big;
  pl->tiles_m_small = t.tm_small;
  pl->n_big = t.tm_big * pl->tiles_n;
  pl->grid[0] = pl->n_big + t.tm_small * pl->tiles_n;
  pl->block = 512;
  pl->lds_bytes = 8 * 64 * 272;      // max(2 x 64 KiB k-tile buffers, 8 x 17 KiB epilogue patches)
  return VITCAP_OK;
}

// gemm_nt_kernel: (32 wm) x (32 wn) tiles, `stages` k-tiles of LDS; grid.y = the k splits
void tiles_nt(const vitcap_gemm_desc* d, int family, int wm, int wn, int stages, GemmPlan* pl) {
  pl->family = family;
  pl->wm = wm; pl->wn = wn; pl->stages = stages;
  pl->tiles_m = (d->M + 32 * wm - 1) / (32 * wm);
  pl->tiles_n = (d->N + 32 * wn - 1) / (32 * wn);
  pl->grid[0] = pl->tiles_m * pl->tiles_n;
  pl->grid[1] = pl->split_k;
  pl->lds_bytes = stages * (32 * wm + 32 * wn) * 64 * 2;
}

// LDS-staged ring: small tiles (decode shapes) 4 stages, 128x128 tiles 2
int plan_ring(const vitcap_gemm_desc* d, const GemmOperands& o, int wm, int wn, int act, int out, GemmPlan* pl) {
  VC_REQUIRE(act >= VITCAP_ACT_NONE && act <= VITCAP_ACT_TANH && (out == VITCAP_OUT_BF16 || out == VITCAP_OUT_F32),
             "gemm: unsupported act %d / out %d", act, out);
  pl->act = act; pl->out_f32 = out; pl->has_res = o.res;
  tiles_nt(d, VITCAP_GEMM_FAMILY_RING, wm, wn, (wm <= 2 && wn <= 2) ? 4 : 2, pl);
  return VITCAP_OK;
}

// "Resident" form for the decode-step shapes (M <= 256 rows, K a multiple of 768): 12 stages = the WHOLE 768-long k range of the
// workgroup is requested by LDS-DMA in the prologue.  K > 768 is cut into K / 768 splits that write fp32 partial slabs
int plan_resident(const vitcap_gemm_desc* d, const GemmOperands& o, int wm, int wn, GemmPlan* pl) {
  const int act = d->act, out = d->out_dtype;
  if (d->K > 768) {                      // partial slabs only
    pl->act = VITCAP_ACT_NONE; pl->out_f32 = 1; pl->has_res = 0;
    pl->split_k = d->K / 768;
    pl->kt_per_split = 12;
    pl->slab = (long long)d->M * d->ldc;
  } else {
    const bool ok = act == VITCAP_ACT_NONE ? (out != 0 || !o.res) : act == VITCAP_ACT_GELU_ERF && !o.res;
    VC_REQUIRE(ok, "gemm(resident): unsupported epilogue act=%d out=%d res=%d", act, out, (int)o.res);
    pl->act = act; pl->out_f32 = out != 0; pl->has_res = o.res;
  }
  tiles_nt(d, VITCAP_GEMM_FAMILY_RESIDENT, wm, wn, 12, pl);
  return VITCAP_OK;
}

// Skinny kernel for split-K decode-step GEMMs: 32-column tiles, blockIdx.z = the split
int plan_skinny(const vitcap_gemm_desc* d, const GemmOperands& o, int split_k, GemmPlan* pl) {
  const int act = d->act, out = d->out_dtype;
  if (split_k > 1) {
    pl->act = VITCAP_ACT_NONE; pl->out_f32 = 1; pl->has_res = 0; pl->partial = 1;
  } else {
    const bool ok = act == VITCAP_ACT_NONE || ((act == VITCAP_ACT_GELU_ERF || act == VITCAP_ACT_TANH) && !o.res);
    VC_REQUIRE(ok, "gemm(skinny): unsupported epilogue act=%d out=%d res=%d", act, out, (int)o.res);
    pl->act = act; pl->out_f32 = out != 0; pl->has_res = o.res;
  }
  pl->family = VITCAP_GEMM_FAMILY_SKINNY;
  pl->wm = d->M <= 64 ? 2 : 4;
  const int bm = 32 * pl->wm, bn = 32 * (4 / pl->wm);
  pl->split_k = split_k;
  pl->kt_per_split = d->K / split_k / 64;
  pl->slab = (long long)d->M * d->ldc;
  pl->grid[0] = (d->N + bn - 1) / bn;
  pl->grid[1] = (d->M + bm - 1) / bm;
  pl->grid[2] = split_k;
  return VITCAP_OK;
}

// Which kernel family runs a large GEMM under tile_hint `hint` (0 = auto, 5 = one tile per workgroup): -1 = the 8-wave kernel of
// gemm.hip, 1 / 2 = the one-tile / persistent form of the 4-wave kernel (gemm4w.hip).  Measured end to end (docs/LAB_r01_r04.md 4.3):
//   auto (one stream): the persistent 4-wave form, +1.8 % images/s at B = 64 and B = 512 against the 8-wave kernel + planned tile mix;
//   tile_hint 5 (the 2-slot pipeline: another stream's small kernels must slip in between tiles): the 8-wave kernel -- a persistent
//   grid owns every CU for the whole GEMM, and a 512-register workgroup leaves no room for a co-resident decode wave (B = 64: 3802
//   vs 3517 img/s) -- except the bf16-output GEMMs without residual (qkv, fc1) below 64k rows, which gain on the 4-wave one-tile
//   form (qkv alone 3 900, fc1 alone 3 907 against 3 856 / 3 866 img/s all 8-wave; proj / fc2 lose: 3 748;
//   profiles/r05_pipeline_gemm_forms.txt).  From 64k rows per launch on that mix is a tie or slightly behind.
int large_gemm_form(int M, int hint, bool plain_bf16) {
  if (M < 2048) return -1;
  if (hint == 0) return 2;
  if (hint == 5) return plain_bf16 && M < 65536 ? 1 : -1;
  return -1;
}

// the tile_hint values vitcap_gemm_ex knows (include/vitcap_hip.h)
bool known_tile_hint(int h) {
  return h == 0 || h == 1 || h == 2 || h == 4 || h == 5 || (h >= 13 && h <= 15) || (h >= 20 && h <= 24) || (h >= 30 && h <= 33) ||
         (h >= 40 && h <= 42);
}

}  // namespace

int vc_gemm_plan(const vitcap_gemm_desc* d, const GemmOperands& o, GemmPlan* pl) {
  *pl = GemmPlan{};
  pl->split_k = 1;
  pl->grid[0] = pl->grid[1] = pl->grid[2] = 1;
  pl->block = 256;
  VC_REQUIRE(d->abi == VITCAP_ABI_VERSION, "gemm: descriptor built against ABI %d, this library is ABI %d", d->abi, VITCAP_ABI_VERSION);
  VC_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "gemm: empty problem M=%d N=%d K=%d", d->M, d->N, d->K);
  VC_REQUIRE(d->K % 64 == 0, "gemm: K=%d must be a multiple of 64", d->K);
  VC_REQUIRE(d->N % 4 == 0 && d->ldc % 4 == 0, "gemm: N=%d and ldc=%d must be multiples of 4", d->N, d->ldc);
  VC_REQUIRE(d->lda % 8 == 0 && d->ldw % 8 == 0, "gemm: lda=%d ldw=%d must be multiples of 8", d->lda, d->ldw);
  VC_REQUIRE(!(o.misaligned & 1), "gemm: A/W/C must be 16-byte aligned");
  VC_REQUIRE(!o.res || (d->ldr % 4 == 0 && !(o.misaligned & 2)), "gemm: residual misaligned");
  VC_REQUIRE(!(o.misaligned & 4), "gemm: bias misaligned");
  VC_REQUIRE(!(o.aux && d->act != VITCAP_ACT_NONE), "gemm: aux (gelu') epilogue needs act == none");
  VC_REQUIRE(!o.zout || d->act == VITCAP_ACT_GELU_ERF, "gemm: zout stores the GELU's derivative and needs act == gelu_erf");
  VC_REQUIRE(known_tile_hint(d->tile_hint), "gemm: unknown tile_hint %d", d->tile_hint);
  const int hint = d->tile_hint;       // the values are listed at vitcap_gemm_desc.tile_hint (include/vitcap_hip.h)
  const int split_k = d->split_k > 1 ? d->split_k : 1;
  const bool plain_rows = d->row_group == 0;
  const bool extras = o.aux || o.zout || d->colsum;
  if (d->ln_out_bf16 || d->ln_out_f32) {
    // LayerNorm of the finished rows: inside the kernel where the launch form has the last-arriver pass, a LayerNorm launch behind
    // the GEMM otherwise -- the same row function either way, so the outputs do not depend on which
    VC_REQUIRE(d->ln_gamma && d->ln_beta, "gemm(ln): ln_gamma / ln_beta missing");
    VC_REQUIRE(d->N == 768 && d->ldc == 768 && d->out_dtype == VITCAP_OUT_F32 && d->act == VITCAP_ACT_NONE && plain_rows && split_k == 1 &&
                   !o.aux && !o.zout && !d->rowstat && !d->colsum,
               "gemm(ln): needs N == ldc == 768, fp32 output, no activation / row remap / split-K / training extras");
    // in-kernel only on request (ln_counters given) and under tile_hint 5 (an fp32 output runs the 8-wave kernel there).  MEASURED A LOSS
    // (docs/LAB_r01_r04.md 4.3: a row block's last arriver pulls its 786 KB back at ~20 GB/s, 40 us per block on one CU, against 31 us
    // for the LayerNorm kernel over ALL rows on the whole chip): the engine does not ask for it
    if (d->ln_counters && d->M >= 2048 && hint == 5) {
      pl->ln_fused = 1;
      return plan_8w(d, o, 0, pl);
    }
    pl->ln_follows = 1;      // the GEMM is routed as if no LayerNorm had been asked for
  }
  if (d->rowstat) {
    // Vocabulary GEMM + row statistics: 64 x 64 tiles for the greedy decode step (M <= 256 rows: weights stream once, most workgroups
    // win), 128 x 128 tiles for beam batches (M = images x beams rows).  Re-measured with the ring's counted waits working
    // (docs/LAB_r01_r04.md 4.2 x): 3 / 6 / 8 stages and 64x128 tiles are all slower than 64x64 x 4 stages in the decode loop
    // (decode phase 5.10-5.18 ms against 5.17-5.26)
    VC_REQUIRE(d->out_dtype == VITCAP_OUT_F32 && d->act == VITCAP_ACT_NONE && !o.res && plain_rows && split_k == 1 && !o.aux && !o.zout,
               "gemm(rowstat): fp32 output, no activation / residual / split-K");
    pl->act = VITCAP_ACT_NONE; pl->out_f32 = 1; pl->has_res = 0;
    if (d->M <= 256) tiles_nt(d, VITCAP_GEMM_FAMILY_ROWSTAT, 2, 2, 4, pl);
    else tiles_nt(d, VITCAP_GEMM_FAMILY_ROWSTAT, 4, 4, 2, pl);
    return VITCAP_OK;
  }
  if (d->colsum) {
    // column sums of the finished bf16 output ride in the 256x256 kernel's 16-byte-store epilogue (training extras build)
    VC_REQUIRE(d->out_dtype == VITCAP_OUT_BF16 && !o.res && plain_rows && split_k == 1 && d->M >= 2048 && d->N % 8 == 0 && d->ldc % 8 == 0 &&
                   (!o.aux || o.ldaux % 8 == 0) && (!o.zout || o.ldz % 8 == 0) && d->act != VITCAP_ACT_TANH,
               "gemm(colsum): needs bf16 output, no residual / row remap / split-K, M >= 2048, N, ldc (ldaux, ldz) multiples of 8");
    // the persistent 4-wave kernel's register epilogue carries the column sums too (round 5), on request only (tile_hint 42): inside
    // the training step it is slower than the 8-wave kernel (profiles/r05_train_extras_ab.txt: 52.2 against 52.5 / 53.1 ms per step)
    if (hint == 42 && supports_4w(d, o, split_k)) return plan_4w(d, o, split_k, 2, pl);
    return plan_8w(d, o, 0, pl);
  }
  if (hint == 23 || hint == 24) {
    // the resident form's contract on the 4-stage ring: K > 768 -> K/768 raw fp32 partial slabs in C = [K/768][M][ldc], one per
    // 768-long k range (blockIdx.y); 64x32 (23) or 32x32 (24) tiles
    VC_REQUIRE(d->K % 768 == 0 && d->K > 768 && plain_rows && !o.aux && !o.zout && d->out_dtype == VITCAP_OUT_F32 && !o.bias && !o.res &&
                   d->act == VITCAP_ACT_NONE,
               "gemm(ring slabs): needs K a multiple of 768 above it, plain rows, raw fp32 slabs (no bias / residual / activation)");
    pl->split_k = d->K / 768;
    pl->kt_per_split = 12;
    pl->slab = (long long)d->M * d->ldc;
    return hint == 23 ? plan_ring(d, o, 2, 1, VITCAP_ACT_NONE, 1, pl) : plan_ring(d, o, 1, 1, VITCAP_ACT_NONE, 1, pl);
  }
  if (hint == 20 || hint == 21 || hint == 22) {
    // resident whole-K form (decode-step shapes); K > 768 -> K/768 fp32 partial slabs in C = [K/768][M][ldc]
    VC_REQUIRE(d->K % 768 == 0 && plain_rows && !o.aux && !o.zout, "gemm(resident): needs K %% 768 == 0, plain rows, no training extras");
    VC_REQUIRE(d->K == 768 || (d->out_dtype == VITCAP_OUT_F32 && !o.bias && !o.res && d->act == VITCAP_ACT_NONE),
               "gemm(resident): K > 768 writes raw fp32 partial slabs");
    if (hint == 20) return plan_resident(d, o, 2, 1, pl);     // 64 x 32 tiles
    if (hint == 21) return plan_resident(d, o, 1, 1, pl);     // 32 x 32
    return plan_resident(d, o, 1, 2, pl);                     // 32 x 64
  }
  if (split_k > 1 && d->M > 256) {
    // weight-gradient shape: few output tiles, very long K -> 128x128 tiles with ragged split-K into fp32 slabs
    VC_REQUIRE(d->out_dtype == VITCAP_OUT_F32 && plain_rows && !o.aux && !o.zout, "gemm: split-K writes fp32 partial slabs only");
    const int nk = d->K / 64;
    pl->split_k = split_k;
    pl->kt_per_split = (nk + split_k - 1) / split_k;
    pl->slab = (long long)d->M * d->ldc;
    return plan_ring(d, o, 4, 4, VITCAP_ACT_NONE, 1, pl);
  }
  if (split_k > 1) {
    VC_REQUIRE(d->K % (128 * split_k) == 0, "gemm: K=%d not divisible into %d splits of multiples of 128", d->K, split_k);
    VC_REQUIRE(d->out_dtype == VITCAP_OUT_F32 && plain_rows, "gemm: split-K writes fp32 partial slabs only");
  }
  // measured at B=64 (tools/decode_bench.py): without split-K the LDS-staged 64x64 kernel is ~2x faster than the
  // register-fed one (7.4 vs 14.6 us for 128x2304x768), so the skinny kernel is used for split-K only.
  if (split_k > 1 || hint == 4) {
    VC_REQUIRE(d->K % 128 == 0 && plain_rows, "gemm(skinny): needs K %% 128 == 0 and no row remap");
    return plan_skinny(d, o, split_k, pl);
  }
  if (hint == 13) return plan_ring(d, o, 2, 1, d->act, d->out_dtype, pl);
  if (hint == 14) return plan_ring(d, o, 1, 1, d->act, d->out_dtype, pl);
  if (hint == 15) return plan_ring(d, o, 1, 2, d->act, d->out_dtype, pl);
  // decode shapes (M = 2 x sequences): weights stream from HBM once, the kernel is latency-bound, so the smallest
  // tiles (most workgroups, most bytes in flight) win: cold-weight 128x2304x768 takes 10.8 / 9.4 / 8.9 us with
  // 64x64 / 64x32 / 32x32 tiles (tools/cold_gemm.py), against a ~4.5 us launch floor
  if (hint == 0 && d->M <= 128) return plan_ring(d, o, 1, 1, d->act, d->out_dtype, pl);
  if (hint == 1 || (hint == 0 && d->M <= 256)) return plan_ring(d, o, 2, 2, d->act, d->out_dtype, pl);
  if (hint == 0 && d->act != VITCAP_ACT_TANH) {
    // Auto tile choice for 256 < M: the tile whose grid costs least under a linear model fitted to tools/gemm_bench.py on the
    // hot shapes (M = 577 .. 36928; N = 768 / 2304 / 3072; K = 768 / 3072; us).  64x64: 4 + W * c; 128x128: max(one tile, 9 + W * c);
    // 256x256: ceil(W / 256) * one tile.  A 256x256 grid of 30 workgroups (N = 768 at 1..8 images) leaves 7/8 of the chip idle
    // for a whole tile time (fc2 at 4 images: 65 us, against 28 us on 64x64 tiles); one image's encoder 3.3 -> 2.6 ms.
    const float kf = d->K > 768 ? (float)(d->K - 768) / 2304.f : 0.f;
    const auto grid = [&](int t) { return (float)(((d->M + t - 1) / t) * ((d->N + t - 1) / t)); };
    const float t64 = 4.f + grid(64) * (0.0165f + kf * 0.0385f);
    const float t128 = fmaxf(16.f + kf * 26.f, 9.f + grid(128) * (0.0375f + kf * 0.0745f));
    const float t256 = d->M >= 2048 ? ceilf(grid(256) / 256.f) * (23.f + kf * 57.f) : 1e30f;
    if (t64 < t128 && t64 < t256) return plan_ring(d, o, 2, 2, d->act, d->out_dtype, pl);
    if (t128 < t256) return plan_ring(d, o, 4, 4, d->act, d->out_dtype, pl);
  }
  if (hint == 2 || (hint == 0 && (d->M < 2048 || d->act == VITCAP_ACT_TANH))) return plan_ring(d, o, 4, 4, d->act, d->out_dtype, pl);
  if (hint >= 40 && hint <= 42) {      // 4 waves x 128x128, one wave per SIMD (gemm4w.hip): 40 LDS epilogue, 41 register epilogue, 42 persistent
    VC_REQUIRE(!extras || (hint == 42 && d->out_dtype == VITCAP_OUT_BF16),
               "gemm(4-wave): aux / zout / colsum need the persistent form (tile_hint 42) and a bf16 output");
    return plan_4w(d, o, split_k, hint - 40, pl);
  }
  if (hint == 30) return plan_8w(d, o, 3, pl);    // every tile 192 x 256 (tile-cost measurement)
  if (hint == 31) return plan_8w(d, o, 2, pl);    // every tile 128 x 256
  if (hint == 32) return plan_8w(d, o, 0, pl);    // 256 x 256 tiles only (no short tail tiles)
  if (hint == 33) return plan_8w(d, o, -1, pl);   // 256-row tiles + the planned short tiles
  // tile_hint 0 (M >= 2048) or 5: the 4-wave kernel where large_gemm_form says so and the launch carries none of the training extras
  // (aux / zout / colsum: the 8-wave kernel's EXTRAS build unless tile_hint 42 asks otherwise), the 8-wave 256x256 kernel otherwise
  const int form = large_gemm_form(d->M, hint, !(d->out_dtype == VITCAP_OUT_F32 || o.res));
  if (form >= 0 && !extras && supports_4w(d, o, split_k)) return plan_4w(d, o, split_k, form, pl);
  // hint 5: 256 x 256 tiles only; auto: short tiles in the last round where the plan wins
  return plan_8w(d, o, hint == 5 ? 0 : -1, pl);
}

extern "C" int vitcap_gemm_plan(const vitcap_gemm_desc* d, int has_bias, int has_residual, int has_aux, int ldaux, int has_zout, int ldz,
                                vitcap_gemm_plan_info* out) {
  VC_REQUIRE(d && out, "gemm: null pointer");
  return vc_gemm_plan(d, GemmOperands{has_bias != 0, has_residual != 0, has_aux != 0, has_zout != 0, ldaux, ldz, 0u}, out);
}

// What the LARGE-TILE family (8-wave / 4-wave 256-column kernels) chooses for a bf16-output GEMM with ldc == N under tile_hint 0 or 5:
// -1 = the 8-wave kernel, otherwise form + 10 * MI of the 4-wave kernel.  Under tile_hint 0 a launch only reaches this family when the
// auto cost model of vc_gemm_plan does not prefer 64x64 or 128x128 tiles; vitcap_gemm_plan reports what a descriptor really launches.
extern "C" int vitcap_gemm_large_form(int M, int N, int K, int tile_hint) {
  // tile_hint | 0x100: the query is about a bf16-output GEMM without residual (under tile_hint 5 those run the 4-wave one-tile form)
  const bool plain_bf16 = (tile_hint & 0x100) != 0;
  const int form = large_gemm_form(M, tile_hint & 0xff, plain_bf16);
  if (form < 0 || K < 128) return -1;                       // supports_4w
  const Form4w f = form_4w(form, M, N, K, N, 0, false, false);
  return f.form + 10 * f.mi;
}

extern "C" int vitcap_gemm_tile_plan(int M, int N, int K, int* plan3) {
  VC_REQUIRE(M > 0 && N > 0 && K > 0 && plan3, "gemm_tile_plan: bad arguments");
  const TilePlan pl = plan_tiles(M, (N + 255) / 256, K);
  plan3[0] = pl.tm_big;
  plan3[1] = pl.mts;
  plan3[2] = pl.tm_small;
  return VITCAP_OK;
}

extern "C" int vitcap_gemm_reserve_cus(int cus) {
  if (cus < 0) cus = 0;
  cus = (cus + 7) & ~7;
  return g_reserve_cus.exchange(cus, std::memory_order_relaxed);
}
