// extern "C" boundary of libmmu_hip.so (declared in include/mmu.h).
// Validates arguments, flattens structs into kernel params, launches on the caller's
// stream, and reports failures through a thread-local message (mmu_last_error).
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <vector>
#include "mmu_internal.h"
#include "plan.h"
#include <cstdlib>
#include <cmath>

using namespace mmu;

static thread_local std::string g_err;

namespace mmu {
const uint64_t* g_seed_off = nullptr;

// deterministic mode (mmu_set_deterministic): host state, read when a launch is chosen.  -1: not
// read yet; the first reader takes MMU_DETERMINISTIC=1 from the environment.
static std::atomic<int> g_det{-1};
bool deterministic() {
  int v = g_det.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("MMU_DETERMINISTIC");
    int want = (e && atoi(e) == 1) ? 1 : 0;
    if (!g_det.compare_exchange_strong(v, want)) want = v;
    v = want;
  }
  return v != 0;
}
}

int mmu_get_deterministic(void) { return mmu::deterministic() ? 1 : 0; }
int mmu_set_deterministic(int on) {
  const int prev = mmu::deterministic() ? 1 : 0;
  mmu::g_det.store(on ? 1 : 0);
  return prev;
}

int mmu_set_seed_offset(const uint64_t* dev_counter) {
  g_seed_off = dev_counter;
  return 0;
}

static int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

// a plan function's refusal (plan.h): its format over the plan's `why` values
static int refused(const char* fmt, const int64_t (&why)[6]) {
  return fail(fmt, why[0], why[1], why[2], why[3], why[4], why[5]);
}

// the conv / stem / pool kernels move 16 B per lane: every tensor they are given must start on a
// 16-B boundary (a NULL optional pointer passes)
static bool off16(const void* q) { return ((uintptr_t)q & 15) != 0; }

static int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("%s: launch failed: %s", what, hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------ timing of mmu_gemm
namespace {
struct Timing {
  std::mutex mu;
  bool on = false;
  bool paused = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool, used;
  std::vector<double> flops;
} g_t;

std::pair<hipEvent_t, hipEvent_t> take_events() {
  std::lock_guard<std::mutex> lk(g_t.mu);
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!g_t.pool.empty()) {
    ev = g_t.pool.back();
    g_t.pool.pop_back();
  } else {
    (void)hipEventCreate(&ev.first);
    (void)hipEventCreate(&ev.second);
  }
  return ev;
}
// per-(device, stream) f32 scratch of mmu_gemm, TAIL_WS_FLOATS (plan.h) per slot, allocated on first
// use outside stream capture (NULL: the product is planned again without that slot)
// (slot 0: the split tail's slabs, slot 1: the column-sum partial rows)
float* tail_workspace(int64_t floats, hipStream_t s, int slot) {
  static std::mutex mu;
  static std::map<std::tuple<int, hipStream_t, int>, float*> bufs;
  if (floats > TAIL_WS_FLOATS) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = bufs.find({dev, s, slot});
  if (it != bufs.end()) return it->second;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
  void* b = nullptr;
  if (hipMalloc(&b, sizeof(float) * TAIL_WS_FLOATS) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  bufs[{dev, s, slot}] = (float*)b;
  return (float*)b;
}
}  // namespace

extern "C" {

int mmu_version(void) { return MMU_ABI_VERSION; }
const char* mmu_last_error(void) { return g_err.c_str(); }

int mmu_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_t.mu);
  g_t.on = on != 0;
  for (auto& e : g_t.used) g_t.pool.push_back(e);
  g_t.used.clear();
  g_t.flops.clear();
  return 0;
}

int mmu_timing_pause(int paused) {
  std::lock_guard<std::mutex> lk(g_t.mu);
  g_t.paused = paused != 0;
  return 0;
}

int mmu_timing_read(double* total_ms, int64_t* launches, double* flops) {
  std::lock_guard<std::mutex> lk(g_t.mu);
  double tot = 0.0, fl = 0.0;
  for (size_t i = 0; i < g_t.used.size(); ++i) {
    (void)hipEventSynchronize(g_t.used[i].second);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_t.used[i].first, g_t.used[i].second) != hipSuccess) return fail("timing: elapsed");
    tot += ms;
    fl += g_t.flops[i];
  }
  *total_ms = tot;
  *launches = (int64_t)g_t.used.size();
  *flops = fl;
  return 0;
}

// the MMU_GEMM_* environment knobs and the deterministic switch of one mmu_gemm call (read per
// call, ~1 us: tests switch them inside one process)
static GemmKnobs gemm_knobs() {
  GemmKnobs kn;
  if (const char* e = getenv("MMU_GEMM_WIDE")) kn.wide_mode = atoi(e);
  if (const char* e = getenv("MMU_GEMM_WIDE_MIN_TILES")) kn.wide_min_tiles = (int64_t)atoll(e);
  if (const char* e = getenv("MMU_GEMM_TAIL")) kn.tail_mode = atoi(e);
  if (const char* e = getenv("MMU_GEMM_CS_PART")) kn.cs_part = atoi(e);
  kn.deterministic = deterministic();
  return kn;
}

// mmu_gemm / mmu_gemm_rows: the dropout counter of row m is that of row drop_row_off + m drop_row_step.
// Validate (pointers, alignment, epilogue combinations), plan (plan.h: the shape rules and every
// choice), take the scratch the plan asks for, launch from the plan.  Nothing is enqueued before
// the last refusal.
static int gemm_impl(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C,
                     int64_t ldc, int c_dtype, int64_t M, int64_t N, int64_t K, int64_t batch, int64_t strideA,
                     int64_t strideB, int64_t strideC, const mmu_epilogue* epi, int64_t drop_row_step,
                     int64_t drop_row_off, mmu_stream_t stream) {
  if (!A || !B || !C) return fail("mmu_gemm: null operand");
  if ((lda % 8) || (ldb % 8) || (ldc % 4)) return fail("mmu_gemm: leading dims must be 16-B aligned");
  if (c_dtype != MMU_BF16 && c_dtype != MMU_F32) return fail("mmu_gemm: bad c_dtype");
  GemmParams p{};
  p.A = (const bf16*)A; p.B = (const bf16*)B; p.C = C;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.sA = strideA; p.sB = strideB; p.sC = strideC;
  p.drop_ldn = N * drop_row_step; p.drop_base = N * drop_row_off;
  int kind = MMU_EPI_STORE;
  if (epi) {
    kind = epi->kind;
    p.accumulate = epi->accumulate;
    p.bias = epi->bias; p.bias_bstride = epi->bias_bstride;
    p.residual = epi->residual; p.ldr = epi->ldr; p.res_bstride = epi->res_bstride;
    p.aux = epi->aux; p.ldx = epi->ldx; p.aux_bstride = epi->aux_bstride;
    p.colsum = epi->colsum; p.colsum_bstride = epi->colsum_bstride;
    p.drop_p = epi->drop_p; p.seed = epi->seed; p.seed_off = g_seed_off;
    p.res_ln_mean = epi->res_ln_mean; p.res_ln_rstd = epi->res_ln_rstd;
    p.res_ln_w = epi->res_ln_w; p.res_ln_b = epi->res_ln_b; p.res_ln_bstride = epi->res_ln_bstride;
    p.bn_x = (const bf16*)epi->bn_x; p.bn_mask = epi->bn_mask; p.bn_mean = epi->bn_mean;
    p.res_mask = epi->res_mask;
  }
  p.kind = kind;
  if (kind < 0 || kind > MMU_EPI_ADD_RES_BNB) return fail("mmu_gemm: bad epilogue kind %d", kind);
  if ((kind == MMU_EPI_STORE_BNB || kind == MMU_EPI_ADD_RES_BNB) &&
      (!p.colsum || !p.bn_x || !p.bn_mean || batch != 1 || !a_kmajor || b_kmajor || p.accumulate || p.bias ||
       ldc != N || c_dtype != MMU_BF16))
    return fail("mmu_gemm: *_BNB needs the table (colsum), bn_x, bn_mean, batch 1, K-major A, N-major B, "
                "bf16 C with ldc == N, no bias / accumulate");
  if (kind == MMU_EPI_STORE_STATS && (!p.colsum || batch != 1 || !a_kmajor || !b_kmajor || p.accumulate))
    return fail("mmu_gemm: STORE_STATS needs the stats table (colsum), batch 1, K-major A and B, no accumulate");
  if (kind != MMU_EPI_STORE && kind != MMU_EPI_BIAS_DROP_RES && c_dtype != MMU_BF16)
    return fail("mmu_gemm: fused epilogues other than BIAS_DROP_RES write bf16");
  if (kind == MMU_EPI_BIAS_DROP_RES && c_dtype == MMU_F32 && (ldc % 4 || (epi && epi->ldr % 4)))
    return fail("mmu_gemm: f32 hidden-stream epilogue needs 16-B aligned rows");
  {
    const int nln = !!p.res_ln_mean + !!p.res_ln_rstd + !!p.res_ln_w + !!p.res_ln_b;
    if (nln && (nln != 4 || kind != MMU_EPI_BIAS_DROP_RES || c_dtype != MMU_F32))
      return fail("mmu_gemm: res_ln_* (all four) only with BIAS_DROP_RES into an f32 C");
  }
  if (kind == MMU_EPI_DGELU && !p.aux) return fail("mmu_gemm: DGELU epilogue needs aux");
  if ((kind == MMU_EPI_BIAS_DROP_RES || kind == MMU_EPI_ADD_RES || kind == MMU_EPI_ADD_RES_BNB) && !p.residual)
    return fail("mmu_gemm: epilogue needs residual");
  if (p.res_mask && ((kind != MMU_EPI_ADD_RES && kind != MMU_EPI_ADD_RES_BNB) || epi->ldr != N || batch != 1))
    return fail("mmu_gemm: res_mask only with ADD_RES / ADD_RES_BNB, batch 1, ldr == N");
  if (p.accumulate && c_dtype != MMU_F32) return fail("mmu_gemm: accumulate needs f32 C");
  if (p.drop_p < 0.f || p.drop_p >= 1.f) return fail("mmu_gemm: drop_p out of range");
  // Every access of the kernels below is a 16-B vector at a column that is a multiple of 8: the
  // operand tiles (uint4 / 16-B buffer loads), C (bf16x8, or two float4), residual and aux rows
  // (bf16x8; float4 for the f32 hidden stream), bias / res_ln_w / res_ln_b / bn_mean (float4) and the
  // float2 tables (float4 per column pair).  So each base, each leading dimension and, for
  // batch > 1, each batch stride must keep 16 B.  (The plain colsum is reached by 4-B atomics and
  // scalar folds only, res_ln_mean / res_ln_rstd by scalar loads, the masks by byte loads.)
  {
    const bool bat = batch > 1;
    auto off16 = [](const void* q) { return ((uintptr_t)q & 15) != 0; };
    const bool cf32 = c_dtype == MMU_F32;
    if (off16(A) || off16(B) || off16(C)) return fail("mmu_gemm: A, B and C must be 16-B aligned");
    if (!cf32 && ldc % 8) return fail("mmu_gemm: ldc=%ld of a bf16 C must be a multiple of 8", ldc);
    if (bat && (strideA % 8 || strideB % 8 || strideC % (cf32 ? 4 : 8)))
      return fail("mmu_gemm: batch strides must keep the operands 16-B aligned");
    const bool uses_res = kind == MMU_EPI_BIAS_DROP_RES || kind == MMU_EPI_ADD_RES || kind == MMU_EPI_ADD_RES_BNB;
    if (uses_res) {
      const int64_t rq = (kind == MMU_EPI_BIAS_DROP_RES && cf32) ? 4 : 8;  // elements per 16 B
      if (off16(p.residual) || p.ldr % rq || (bat && p.res_bstride % rq))
        return fail("mmu_gemm: residual, ldr=%ld and res_bstride must keep 16-B alignment", p.ldr);
    }
    const bool uses_aux = p.aux && (kind == MMU_EPI_BIAS_GELU || kind == MMU_EPI_DGELU || kind == MMU_EPI_BIAS_DROP_QGELU);
    if (uses_aux && (off16(p.aux) || p.ldx % 8 || (bat && p.aux_bstride % 8)))
      return fail("mmu_gemm: aux, ldx=%ld and aux_bstride must keep 16-B alignment", p.ldx);
    const bool uses_bias = p.bias && kind != MMU_EPI_DGELU && kind != MMU_EPI_ADD_RES;
    if (uses_bias && (off16(p.bias) || (bat && p.bias_bstride % 4)))
      return fail("mmu_gemm: bias and bias_bstride must keep 16-B alignment");
    if (p.res_ln_w && (off16(p.res_ln_w) || off16(p.res_ln_b) || (bat && p.res_ln_bstride % 4)))
      return fail("mmu_gemm: res_ln_w, res_ln_b and res_ln_bstride must keep 16-B alignment");
    if (p.res_ln_w && (((uintptr_t)p.res_ln_mean | (uintptr_t)p.res_ln_rstd) & 3))
      return fail("mmu_gemm: res_ln_mean / res_ln_rstd must be 4-B aligned");
    const bool table = kind == MMU_EPI_STORE_STATS || kind == MMU_EPI_STORE_BNB || kind == MMU_EPI_ADD_RES_BNB;
    if (table && off16(p.colsum)) return fail("mmu_gemm: the float2 table (colsum) must be 16-B aligned");
    if (!table && p.colsum && ((uintptr_t)p.colsum & 3)) return fail("mmu_gemm: colsum must be 4-B aligned");
    if (epi && epi->workspace && off16(epi->workspace))
      return fail("mmu_gemm: the split-K workspace must be 16-B aligned (float4 slabs)");
    if ((kind == MMU_EPI_STORE_BNB || kind == MMU_EPI_ADD_RES_BNB) && (off16(p.bn_x) || off16(p.bn_mean)))
      return fail("mmu_gemm: bn_x and bn_mean must be 16-B aligned");
  }
  // ---- plan, assuming both scratch slots can be had; then take only the scratch the plan asks
  // for, and plan again without a slot that cannot be had (first use under stream capture, a
  // failed hipMalloc): no tail scratch -> no tail split, no column-sum scratch -> atomics, or the
  // deterministic refusal
  hipStream_t s = (hipStream_t)stream;
  const GemmShape shape{M, N, K, batch, lda, ldb, a_kmajor != 0, b_kmajor != 0, c_dtype == MMU_F32, kind,
                        p.bias != nullptr, p.colsum != nullptr, (epi && epi->workspace) ? epi->workspace_floats : 0};
  const GemmKnobs knobs = gemm_knobs();
  GemmScratch scratch{TAIL_WS_FLOATS, TAIL_WS_FLOATS};
  GemmPlan pl;
  const char* no = gemm_plan(shape, knobs, scratch, pl);
  float *tail_ws = nullptr, *cs_part = nullptr;
  if (!no && pl.tail_rows && !(tail_ws = tail_workspace(pl.tail_split * pl.tail_rows * N, s, 0))) {
    scratch.tail_floats = 0;
    no = gemm_plan(shape, knobs, scratch, pl);
  }
  if (!no && pl.cs == CS_ROWS && !(cs_part = tail_workspace(pl.cs_parts * N, s, 1))) {
    scratch.cs_floats = 0;
    no = gemm_plan(shape, knobs, scratch, pl);
  }
  if (no) return refused(no, pl.why);
  // ---- launch from the plan
  p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.group_m = pl.group_m;
  p.splitk = pl.splitk; p.kchunk = pl.kchunk;
  if (pl.splitk > 1) p.ws = epi->workspace;
  const int64_t cs_parts_main = pl.cs_parts - (pl.tail_rows + 63) / 64;
  if (cs_part) {
    p.cs_part = cs_part;
    p.cs_m0 = 0;
    p.cs_rows = pl.cs_rows;
  }
  const bool f32out = c_dtype == MMU_F32;
  bool timed;
  std::pair<hipEvent_t, hipEvent_t> ev;
  {
    std::lock_guard<std::mutex> lk(g_t.mu);
    timed = g_t.on && !g_t.paused;
  }
  if (timed) {
    ev = take_events();
    (void)hipEventRecord(ev.first, s);
  }
  {
    GemmParams pm = p;  // the main tiling: every tile row, or those above the split tail rows
    if (pl.tail_rows) pm.tiles_m = (int)(pl.m_main / 256);
    if (pl.tiling != GEMM_WIDE)
      gemm_launch(pm, a_kmajor != 0, b_kmajor != 0, f32out, pl.tiling == GEMM_BIG, (int)batch, s);
    else if (!gemm_wide_launch(pm, f32out, (int)batch, s))
      return fail("mmu_gemm: internal error: the plan chose the 256 x 384 tiling for epilogue kind %d", kind);
  }
  if (pl.tail_rows) {
    GemmParams pt = p;  // the tail rows' K slices: raw partial products of the small tiling
    pt.A = p.A + pl.m_main * lda;
    pt.M = pl.tail_rows;
    pt.kind = MMU_EPI_STORE;
    pt.accumulate = 0;
    pt.splitk = pl.tail_split;
    pt.kchunk = pl.tail_chunk;
    pt.ws = tail_ws;
    pt.tiles_m = (int)((pl.tail_rows + 127) / 128);
    pt.tiles_n = (int)(N / 128);
    pt.group_m = 1;
    pt.cs_part = nullptr;
    gemm_launch(pt, true, b_kmajor != 0, true, false, 1, s);
    GemmParams pe = p;  // their sum and epilogue
    if (cs_part) {
      pe.cs_part = cs_part + cs_parts_main * N;
      pe.cs_m0 = pl.m_main;
      pe.cs_rows = 64;
    }
    if (!splitk_epilogue_launch(pe, f32out, tail_ws, pl.m_main, pl.tail_rows, pl.tail_split, s))
      return fail("mmu_gemm: internal error: the plan split the tail rows of epilogue kind %d", kind);
  }
  if (cs_part) colsum_reduce_launch(cs_part, pl.cs_parts, N, p.colsum, 1, s);
  if (pl.splitk > 1) splitk_reduce_launch(p, (int)batch, s);
  if (timed) {
    (void)hipEventRecord(ev.second, s);
    std::lock_guard<std::mutex> lk(g_t.mu);
    g_t.used.push_back(ev);
    g_t.flops.push_back(2.0 * (double)M * (double)N * (double)K * (double)batch);
  }
  return check_launch("mmu_gemm");
}

// the plan mmu_gemm would follow: the same knobs, through the same plan function, with both scratch
// slots assumed available; no HIP call
int mmu_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t batch, int64_t lda, int64_t ldb, int a_kmajor,
                  int b_kmajor, int c_dtype, int kind, int has_bias, int has_colsum, int64_t workspace_floats,
                  int64_t* plan) {
  if (!plan) return fail("mmu_gemm_plan: null plan");
  if (c_dtype != MMU_BF16 && c_dtype != MMU_F32) return fail("mmu_gemm_plan: bad c_dtype");
  if (kind < 0 || kind > MMU_EPI_ADD_RES_BNB) return fail("mmu_gemm_plan: bad epilogue kind %d", kind);
  const GemmShape shape{M, N, K, batch, lda, ldb, a_kmajor != 0, b_kmajor != 0, c_dtype == MMU_F32, kind,
                        has_bias != 0, has_colsum != 0, workspace_floats};
  GemmPlan pl;
  if (const char* no = gemm_plan(shape, gemm_knobs(), GemmScratch{TAIL_WS_FLOATS, TAIL_WS_FLOATS}, pl))
    return refused(no, pl.why);
  const int64_t out[MMU_GEMM_PLAN_FIELDS] = {pl.tiling,    pl.tiles_m,    pl.tiles_n, pl.group_m, pl.splitk,
                                             pl.kchunk,    pl.m_main,     pl.tail_rows, pl.tail_split,
                                             pl.tail_chunk, pl.cs,        pl.cs_rows, pl.cs_parts};
  for (int i = 0; i < MMU_GEMM_PLAN_FIELDS; ++i) plan[i] = out[i];
  return 0;
}


int mmu_gemm(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C,
             int64_t ldc, int c_dtype, int64_t M, int64_t N, int64_t K, int64_t batch, int64_t strideA,
             int64_t strideB, int64_t strideC, const mmu_epilogue* epi, mmu_stream_t stream) {
  return gemm_impl(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, c_dtype, M, N, K, batch, strideA, strideB, strideC, epi,
                   1, 0, stream);
}

int mmu_gemm_rows(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C,
                  int64_t ldc, int c_dtype, int64_t M, int64_t N, int64_t K, int64_t batch, int64_t strideA,
                  int64_t strideB, int64_t strideC, const mmu_epilogue* epi, int64_t drop_row_step,
                  int64_t drop_row_offset, mmu_stream_t stream) {
  if (drop_row_step < 1 || drop_row_offset < 0) return fail("mmu_gemm_rows: drop_row_step >= 1, drop_row_offset >= 0");
  return gemm_impl(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, c_dtype, M, N, K, batch, strideA, strideB, strideC, epi,
                   drop_row_step, drop_row_offset, stream);
}

int mmu_transpose_bf16_batched(const int64_t* jobs, int n_jobs, int64_t max_rows, int64_t max_cols,
                               mmu_stream_t stream) {
  if (!jobs || n_jobs <= 0 || n_jobs > 65535 || max_rows <= 0 || max_cols <= 0)
    return fail("mmu_transpose_bf16_batched: bad args");
  transpose_bf16_batched_launch(jobs, n_jobs, max_rows, max_cols, (hipStream_t)stream);
  return check_launch("mmu_transpose_bf16_batched");
}

int mmu_colsum_reduce(const float* partial, int64_t parts, int64_t N, float* out, int accumulate,
                      mmu_stream_t stream) {
  if (!partial || !out || parts <= 0 || N <= 0) return fail("mmu_colsum_reduce: bad args");
  colsum_reduce_launch(partial, parts, N, out, accumulate, (hipStream_t)stream);
  return check_launch("mmu_colsum_reduce");
}

int mmu_colsum_reduce_multi(int n, const float* const* partial, const int64_t* parts, float* const* out, int64_t N,
                            int accumulate, mmu_stream_t stream) {
  if (n <= 0 || n > COLSUM_MULTI || !partial || !parts || !out || N <= 0)
    return fail("mmu_colsum_reduce_multi: bad args (1 <= n <= %d)", COLSUM_MULTI);
  ColsumJobs jobs{};
  for (int z = 0; z < n; ++z) {
    if (!partial[z] || !out[z] || parts[z] <= 0) return fail("mmu_colsum_reduce_multi: bad job %d", z);
    jobs.part[z] = partial[z];
    jobs.parts[z] = parts[z];
    jobs.out[z] = out[z];
  }
  colsum_reduce_multi_launch(jobs, n, N, accumulate, (hipStream_t)stream);
  return check_launch("mmu_colsum_reduce_multi");
}

int mmu_colsum_bf16(const void* X, int64_t M, int64_t N, int64_t ldx, float* partial, float* out, int accumulate,
                    mmu_stream_t stream) {
  if (!X || !out || M <= 0 || N <= 0 || N % 8 || ldx % 8) return fail("mmu_colsum_bf16: bad args");
  if (deterministic() && !partial && M > colsum_bf16_rows_max())
    return fail("mmu_colsum_bf16: deterministic mode: M=%ld spans more than one row block and needs the scratch table",
                M);
  colsum_bf16_launch((const bf16*)X, M, N, ldx, partial, out, accumulate, (hipStream_t)stream);
  return check_launch("mmu_colsum_bf16");
}

static int attn_common(int64_t ld_qkv, int64_t batch, int64_t L, int64_t heads, float drop_p) {
  if (batch <= 0 || L <= 0 || heads <= 0) return fail("attention: bad shape");
  if (ld_qkv < 3 * heads * 64 || ld_qkv % 8) return fail("attention: ld_qkv too small / unaligned");
  if (drop_p < 0.f || drop_p >= 1.f) return fail("attention: drop_p out of range");
  if ((int64_t)batch * heads > 65535 * 64) return fail("attention: batch*heads too large");
  if (L > 576) return fail("attention: L=%ld > 576 (the kernels stage ceil(L/64) <= 9 key tiles)", L);
  return 0;
}

int mmu_attention_fwd(const void* QKV, int64_t ld_qkv, const float* keymask, void* O, int64_t ld_o, float* LSE,
                      int64_t batch, int64_t L, int64_t heads, float drop_p, uint64_t seed, uint64_t* dropmask,
                      mmu_stream_t stream) {
  if (!QKV || !keymask || !O || !LSE) return fail("mmu_attention_fwd: null pointer");
  if (attn_common(ld_qkv, batch, L, heads, drop_p)) return 1;
  if (ld_o < heads * 64 || ld_o % 8) return fail("mmu_attention_fwd: bad ld_o");
  if (batch * heads > 65535) return fail("mmu_attention_fwd: batch*heads > 65535");
  AttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv; p.keymask = keymask; p.out = (bf16*)O; p.ld_out = ld_o;
  p.lse = LSE; p.batch = (int)batch; p.L = (int)L; p.heads = (int)heads; p.drop_p = drop_p; p.seed = seed;
  p.seed_off = g_seed_off;
  p.dropmask = dropmask;
  attention_fwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_attention_fwd");
}

int mmu_attention_bwd(const void* QKV, int64_t ld_qkv, const float* keymask, const void* O, int64_t ld_o,
                      const void* dO, int64_t ld_do, const float* LSE, float* delta, void* dQKV, int64_t ld_dqkv,
                      int64_t batch, int64_t L, int64_t heads, float drop_p, uint64_t seed,
                      const uint64_t* dropmask, float* dbias_parts, mmu_stream_t stream) {
  if (!QKV || !keymask || !O || !dO || !LSE || !delta || !dQKV) return fail("mmu_attention_bwd: null pointer");
  if ((uint32_t)(drop_p * 65536.0f + 0.5f) != 0 && !dropmask)
    return fail("mmu_attention_bwd: dropout needs the forward's dropmask");
  if (attn_common(ld_qkv, batch, L, heads, drop_p)) return 1;
  // (ld_o / ld_do below the row width: rows would overlap and the last one be read past the buffer)
  if (ld_dqkv < 3 * heads * 64 || ld_do < heads * 64 || ld_o < heads * 64 || ld_do % 8 || ld_o % 8 || ld_dqkv % 4)
    return fail("mmu_attention_bwd: bad ld");
  if (batch * heads > 65535) return fail("mmu_attention_bwd: batch*heads > 65535");
  AttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv; p.keymask = keymask; p.o = (const bf16*)O; p.ld_o = ld_o;
  p.dout = (const bf16*)dO; p.ld_do = ld_do; p.lse = (float*)LSE; p.delta = delta; p.out = (bf16*)dQKV;
  p.ld_out = ld_dqkv; p.batch = (int)batch; p.L = (int)L; p.heads = (int)heads; p.drop_p = drop_p; p.seed = seed;
  p.seed_off = g_seed_off;
  p.dropmask = (uint64_t*)dropmask;
  p.colsum = dbias_parts;
  attention_bwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_attention_bwd");
}

int mmu_attention_row0_fwd(const void* QKV, int64_t ld_qkv, const float* keymask, void* O, int64_t ld_o, float* LSE,
                           int64_t batch, int64_t L, int64_t heads, float drop_p, uint64_t seed, uint64_t* dropmask,
                           mmu_stream_t stream) {
  if (!QKV || !keymask || !O || !LSE) return fail("mmu_attention_row0_fwd: null pointer");
  if (attn_common(ld_qkv, batch, L, heads, drop_p)) return 1;
  if (ld_o < heads * 64 || ld_o % 8) return fail("mmu_attention_row0_fwd: bad ld_o");
  if (((uintptr_t)QKV | (uintptr_t)O) & 15) return fail("mmu_attention_row0_fwd: QKV / O must be 16-B aligned");
  AttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv; p.keymask = keymask; p.out = (bf16*)O; p.ld_out = ld_o;
  p.lse = LSE; p.batch = (int)batch; p.L = (int)L; p.heads = (int)heads; p.drop_p = drop_p; p.seed = seed;
  p.seed_off = g_seed_off;
  p.dropmask = dropmask;
  attention_row0_fwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_attention_row0_fwd");
}

int mmu_attention_row0_bwd(const void* QKV, int64_t ld_qkv, const float* keymask, const void* O, int64_t ld_o,
                           const void* dO, int64_t ld_do, const float* LSE, void* dQKV, int64_t ld_dqkv,
                           int64_t batch, int64_t L, int64_t heads, float drop_p, const uint64_t* dropmask,
                           float* dbias_sums, mmu_stream_t stream) {
  if (!QKV || !keymask || !O || !dO || !LSE || !dQKV) return fail("mmu_attention_row0_bwd: null pointer");
  if ((uint32_t)(drop_p * 65536.0f + 0.5f) != 0 && !dropmask)
    return fail("mmu_attention_row0_bwd: dropout needs the forward's dropmask");
  if (attn_common(ld_qkv, batch, L, heads, drop_p)) return 1;
  if (ld_dqkv < 3 * heads * 64 || ld_do < heads * 64 || ld_o < heads * 64 || ld_do % 8 || ld_o % 8 || ld_dqkv % 8)
    return fail("mmu_attention_row0_bwd: bad ld");
  if (((uintptr_t)QKV | (uintptr_t)O | (uintptr_t)dO | (uintptr_t)dQKV) & 15)
    return fail("mmu_attention_row0_bwd: QKV / O / dO / dQKV must be 16-B aligned");
  AttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv; p.keymask = keymask; p.o = (const bf16*)O; p.ld_o = ld_o;
  p.dout = (const bf16*)dO; p.ld_do = ld_do; p.lse = (float*)LSE; p.out = (bf16*)dQKV;
  p.ld_out = ld_dqkv; p.batch = (int)batch; p.L = (int)L; p.heads = (int)heads; p.drop_p = drop_p;
  p.dropmask = (uint64_t*)dropmask;
  p.colsum = dbias_sums;
  attention_row0_bwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_attention_row0_bwd");
}

int mmu_layernorm_fwd(const void* X, const float* w, const float* b, void* Y, float* mean, float* rstd, int64_t rows,
                      int64_t H, float eps, int64_t group_rows, int64_t param_stride, mmu_stream_t stream) {
  if (!X || !w || !b || !Y) return fail("mmu_layernorm_fwd: null pointer");
  if ((mean == nullptr) != (rstd == nullptr)) return fail("mmu_layernorm_fwd: mean/rstd must both be given or NULL");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024) return fail("mmu_layernorm_fwd: H=%ld must be 256/512/768/1024", H);
  if (group_rows <= 0) group_rows = rows;
  if (param_stride < 0) return fail("mmu_layernorm_fwd: bad param_stride");
  layernorm_fwd_launch((const bf16*)X, w, b, (bf16*)Y, mean, rstd, rows, H, eps, group_rows, param_stride,
                       (hipStream_t)stream);
  return check_launch("mmu_layernorm_fwd");
}

int mmu_layernorm_bwd(const void* dY, const void* X, const float* mean, const float* rstd, const float* w, void* dX,
                      void* dXdrop, float drop_p, uint64_t seed, float* part_dw, float* part_db, float* part_dbias,
                      int64_t rows, int64_t H, int64_t rows_per_part, mmu_stream_t stream) {
  if (!dY || !X || !mean || !rstd || !w || !dX) return fail("mmu_layernorm_bwd: null pointer");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024 || rows_per_part <= 0) return fail("mmu_layernorm_bwd: bad shape");
  if (drop_p < 0.f || drop_p >= 1.f) return fail("mmu_layernorm_bwd: drop_p out of range");
  layernorm_bwd_launch((const bf16*)dY, X, false, mean, rstd, w, (bf16*)dX, (bf16*)dXdrop, nullptr, drop_p, seed,
                       g_seed_off, part_dw, part_db, part_dbias, rows, H, rows_per_part, (hipStream_t)stream);
  return check_launch("mmu_layernorm_bwd");
}

int mmu_layernorm_fwd_f32(const float* X, const float* w, const float* b, void* Y, float* Y32, float* mean,
                          float* rstd, int64_t rows, int64_t H, float eps, int64_t group_rows, int64_t param_stride,
                          mmu_stream_t stream) {
  if (!X || !w || !b || !Y) return fail("mmu_layernorm_fwd_f32: null pointer");
  if ((mean == nullptr) != (rstd == nullptr)) return fail("mmu_layernorm_fwd_f32: mean/rstd must both be given or NULL");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024) return fail("mmu_layernorm_fwd_f32: H=%ld must be 256/512/768/1024", H);
  if (group_rows <= 0) group_rows = rows;
  if (param_stride < 0) return fail("mmu_layernorm_fwd_f32: bad param_stride");
  layernorm_fwd32_launch(X, w, b, (bf16*)Y, Y32, mean, rstd, rows, H, eps, group_rows, param_stride,
                         (hipStream_t)stream);
  return check_launch("mmu_layernorm_fwd_f32");
}

int mmu_layernorm_bwd_f32(const void* dY, const float* X, const float* mean, const float* rstd, const float* w,
                          void* dX, void* dXdrop, float drop_p, uint64_t seed, float* part_dw, float* part_db,
                          float* part_dbias, int64_t rows, int64_t H, int64_t rows_per_part, mmu_stream_t stream) {
  if (!dY || !X || !mean || !rstd || !w || !dX) return fail("mmu_layernorm_bwd_f32: null pointer");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024 || rows_per_part <= 0) return fail("mmu_layernorm_bwd_f32: bad shape");
  if (drop_p < 0.f || drop_p >= 1.f) return fail("mmu_layernorm_bwd_f32: drop_p out of range");
  layernorm_bwd_launch((const bf16*)dY, X, true, mean, rstd, w, (bf16*)dX, (bf16*)dXdrop, nullptr, drop_p, seed,
                       g_seed_off, part_dw, part_db, part_dbias, rows, H, rows_per_part, (hipStream_t)stream);
  return check_launch("mmu_layernorm_bwd_f32");
}

int mmu_layernorm_bwd_f32_rows(const void* dY, const float* X, const float* mean, const float* rstd, const float* w,
                               void* dX, void* dXdrop, float drop_p, uint64_t seed, float* part_dw, float* part_db,
                               float* part_dbias, int64_t rows, int64_t H, int64_t rows_per_part,
                               int64_t drop_row_step, int64_t drop_row_offset, mmu_stream_t stream) {
  if (!dY || !X || !mean || !rstd || !w || !dX) return fail("mmu_layernorm_bwd_f32_rows: null pointer");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024 || rows_per_part <= 0)
    return fail("mmu_layernorm_bwd_f32_rows: bad shape");
  if (drop_p < 0.f || drop_p >= 1.f) return fail("mmu_layernorm_bwd_f32_rows: drop_p out of range");
  if (drop_row_step < 1 || drop_row_offset < 0)
    return fail("mmu_layernorm_bwd_f32_rows: drop_row_step >= 1, drop_row_offset >= 0");
  layernorm_bwd_launch((const bf16*)dY, X, true, mean, rstd, w, (bf16*)dX, (bf16*)dXdrop, nullptr, drop_p, seed,
                       g_seed_off, part_dw, part_db, part_dbias, rows, H, rows_per_part, (hipStream_t)stream,
                       drop_row_step, drop_row_offset);
  return check_launch("mmu_layernorm_bwd_f32_rows");
}

int mmu_layernorm_bwd_res(const void* dY, const void* X, const float* mean, const float* rstd, const float* w,
                          const void* dRes, void* dX, float* part_dw, float* part_db, float* part_dbias, int64_t rows,
                          int64_t H, int64_t rows_per_part, mmu_stream_t stream) {
  if (!dY || !X || !mean || !rstd || !w || !dX || !dRes) return fail("mmu_layernorm_bwd_res: null pointer");
  if (rows <= 0 || H <= 0 || H % 256 || H > 1024 || rows_per_part <= 0) return fail("mmu_layernorm_bwd_res: bad shape");
  layernorm_bwd_launch((const bf16*)dY, X, false, mean, rstd, w, (bf16*)dX, nullptr, (const bf16*)dRes, 0.f, 0,
                       nullptr, part_dw, part_db, part_dbias, rows, H, rows_per_part, (hipStream_t)stream);
  return check_launch("mmu_layernorm_bwd_res");
}

static int seqattn_check(const char* what, int64_t ld_qkv, int64_t S, int64_t N, int64_t heads, int64_t D) {
  if (S <= 0 || N <= 0 || heads <= 0) return fail("%s: bad shape", what);
  if (D != 64 && D != 128 && D != 256) return fail("%s: head_dim %ld not in {64, 128, 256}", what, D);
  if (ld_qkv < 3 * heads * D || ld_qkv % 8) return fail("%s: ld_qkv too small / unaligned", what);
  if (N * heads > 65535) return fail("%s: N*heads > 65535", what);
  // the kernels count rows and 64-row tiles in int: the last tile's end, ceil(S/64)*64, must fit
  if (S > (int64_t)INT32_MAX - 63)
    return fail("%s: S = %ld exceeds %ld (INT32_MAX - 63: rows and 64-row tiles are counted in int)", what, S,
                (int64_t)INT32_MAX - 63);
  return 0;
}

// the 16-B row loads (QKV, dO), 8-B row stores (O, dQKV) and f32 vectors (LSE2, delta) of flava.hip
static int seqattn_aligned(const char* what, const char* name, const void* q, int bytes) {
  if ((uintptr_t)q & (uintptr_t)(bytes - 1))
    return fail("%s: %s = %p must be %d-byte aligned", what, name, q, bytes);
  return 0;
}

int mmu_seqattn_fwd(const void* QKV, int64_t ld_qkv, void* O, int64_t ld_o, float* LSE2, int64_t S, int64_t N,
                    int64_t heads, int64_t head_dim, mmu_stream_t stream) {
  if (!QKV || !O || !LSE2) return fail("mmu_seqattn_fwd: null pointer");
  if (seqattn_check("mmu_seqattn_fwd", ld_qkv, S, N, heads, head_dim)) return 1;
  if (ld_o < heads * head_dim || ld_o % 4) return fail("mmu_seqattn_fwd: bad ld_o");
  if (seqattn_aligned("mmu_seqattn_fwd", "QKV", QKV, 16) || seqattn_aligned("mmu_seqattn_fwd", "O", O, 8) ||
      seqattn_aligned("mmu_seqattn_fwd", "LSE2", LSE2, 4))
    return 1;
  SeqAttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv;
  p.out = (bf16*)O; p.ld_out = ld_o;
  p.lse2 = LSE2;
  p.S = (int)S; p.N = (int)N; p.heads = (int)heads; p.D = (int)head_dim; p.E = (int)(heads * head_dim);
  p.scale = 1.0f / sqrtf((float)head_dim);
  seqattn_fwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_seqattn_fwd");
}

int mmu_seqattn_bwd(const void* QKV, int64_t ld_qkv, const void* O, int64_t ld_o, const void* dO, int64_t ld_do,
                    const float* LSE2, float* delta, void* dQKV, int64_t ld_dqkv, int64_t S, int64_t N, int64_t heads,
                    int64_t head_dim, mmu_stream_t stream) {
  if (!QKV || !O || !dO || !LSE2 || !delta || !dQKV) return fail("mmu_seqattn_bwd: null pointer");
  if (seqattn_check("mmu_seqattn_bwd", ld_qkv, S, N, heads, head_dim)) return 1;
  if (ld_dqkv < 3 * heads * head_dim || ld_dqkv % 4 || ld_o % 4 || ld_do % 8) return fail("mmu_seqattn_bwd: bad ld");
  if (ld_o < heads * head_dim)
    return fail("mmu_seqattn_bwd: ld_o = %ld is smaller than heads*head_dim = %ld", ld_o, heads * head_dim);
  if (ld_do < heads * head_dim)
    return fail("mmu_seqattn_bwd: ld_do = %ld is smaller than heads*head_dim = %ld", ld_do, heads * head_dim);
  const char* const who = "mmu_seqattn_bwd";
  if (seqattn_aligned(who, "QKV", QKV, 16) || seqattn_aligned(who, "dO", dO, 16) || seqattn_aligned(who, "O", O, 8) ||
      seqattn_aligned(who, "dQKV", dQKV, 8) || seqattn_aligned(who, "LSE2", LSE2, 4) ||
      seqattn_aligned(who, "delta", delta, 4))
    return 1;
  // the delta kernel's grid: one block per 4 (row, head) items, in the grid's x dimension
  if ((S * N * heads + 3) / 4 > (int64_t)INT32_MAX)
    return fail("mmu_seqattn_bwd: S*N*heads = %ld needs more than %ld delta blocks (the grid's x limit)",
                S * N * heads, (int64_t)INT32_MAX);
  SeqAttnParams p{};
  p.qkv = (const bf16*)QKV; p.ld_qkv = ld_qkv;
  p.o = (const bf16*)O; p.ld_o = ld_o;
  p.dout = (const bf16*)dO; p.ld_do = ld_do;
  p.out = (bf16*)dQKV; p.ld_out = ld_dqkv;
  p.lse2 = (float*)LSE2; p.delta = delta;
  p.S = (int)S; p.N = (int)N; p.heads = (int)heads; p.D = (int)head_dim; p.E = (int)(heads * head_dim);
  p.scale = 1.0f / sqrtf((float)head_dim);
  seqattn_bwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_seqattn_bwd");
}


int mmu_embed_fwd(const int64_t* ids, const int64_t* seg, const int64_t* txt_mask, const float* proj, const float* word,
                  const float* pos, const float* type, const float* ln_w, const float* ln_b, float eps, int64_t cls_id,
                  int64_t sep_id, const int64_t* idx, int64_t V, int64_t B, int64_t T, int64_t n_img, int64_t Lout,
                  int64_t H, float drop_txt, float drop_img, uint64_t seed, void* X, float* X32, float* keymask,
                  float* mean, float* rstd, mmu_stream_t stream) {
  if (H != 768 && H != 1024) return fail("mmu_embed_fwd: H must be 768 or 1024");
  if (!word || !pos || !type || !ln_w || !ln_b || !X || !keymask || !proj) return fail("mmu_embed_fwd: null pointer");
  if (T > 0 && (!ids || !seg)) return fail("mmu_embed_fwd: text ids/segments missing");
  if (V <= 0 || B <= 0 || Lout <= 0 || n_img <= 0) return fail("mmu_embed_fwd: bad shape");
  if (!idx && Lout != n_img + 2 + T) return fail("mmu_embed_fwd: identity variant needs Lout == n_img+2+T");
  EmbedParams p{};
  p.ids = ids; p.seg = seg; p.txt_mask = txt_mask; p.idx = idx; p.proj = proj; p.word = word; p.pos = pos;
  p.type = type; p.ln_w = ln_w; p.ln_b = ln_b; p.eps = eps; p.cls_id = cls_id; p.sep_id = sep_id; p.V = V; p.B = B;
  p.T = T; p.n_img = n_img; p.Lout = Lout; p.H = H; p.X = (bf16*)X; p.X32 = X32;
  if (drop_txt < 0.f || drop_txt >= 1.f || drop_img < 0.f || drop_img >= 1.f) return fail("mmu_embed_fwd: bad dropout");
  p.drop_txt = drop_txt; p.drop_img = drop_img; p.seed = seed; p.seed_off = g_seed_off; p.keymask = keymask; p.mean = mean; p.rstd = rstd;
  embed_fwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_embed_fwd");
}

int64_t mmu_embed_bwd_ws_floats_h(int64_t B, int64_t T, int64_t n_img, int64_t H) {
  if (H != 768 && H != 1024) return -1;
  const int64_t base = 4 * embed_bwd_blocks(B, n_img + 2 + T) * H;
  return deterministic() ? base + embed_bwd_det_ws_floats(B, T, n_img, H) : base;
}

int64_t mmu_embed_bwd_ws_floats(int64_t B, int64_t T, int64_t n_img) { return mmu_embed_bwd_ws_floats_h(B, T, n_img, 768); }

int64_t mmu_embed_bwd_det_chunk(void) { return embed_bwd_det_chunk(); }

int mmu_embed_bwd(const void* dX, const int64_t* ids, const int64_t* seg, const float* proj, const float* word,
                  const float* pos, const float* type, const float* ln_w, const float* mean, const float* rstd,
                  int64_t cls_id, int64_t sep_id, int64_t B, int64_t T, int64_t n_img, int64_t H, float drop_txt,
                  float drop_img, uint64_t seed, float* d_word,
                  float* d_pos, float* d_type, float* d_ln_w, float* d_ln_b, float* d_proj, float* ws,
                  mmu_stream_t stream) {
  if (H != 768 && H != 1024) return fail("mmu_embed_bwd: H must be 768 or 1024");
  if (!dX || !ids || !seg || !proj || !word || !pos || !type || !ln_w || !mean || !rstd || !d_word || !d_pos ||
      !d_type || !d_ln_w || !d_ln_b || !d_proj || !ws)
    return fail("mmu_embed_bwd: null pointer");
  EmbedBwdParams q{};
  q.dX = (const bf16*)dX; q.ids = ids; q.seg = seg; q.proj = proj; q.word = word; q.pos = pos; q.type = type;
  q.ln_w = ln_w; q.mean = mean; q.rstd = rstd; q.cls_id = cls_id; q.sep_id = sep_id; q.B = B; q.T = T;
  q.n_img = n_img; q.H = H; q.drop_txt = drop_txt; q.drop_img = drop_img; q.seed = seed; q.seed_off = g_seed_off; q.d_word = d_word; q.d_pos = d_pos; q.d_type = d_type; q.d_ln_w = d_ln_w;
  q.d_ln_b = d_ln_b; q.d_proj = d_proj; q.ws = ws;
  if (deterministic()) {
    if ((uintptr_t)ws & 15) return fail("mmu_embed_bwd: deterministic mode: ws must be 16-B aligned");
    if (B * T >= (1ll << 31)) return fail("mmu_embed_bwd: deterministic mode: B*T must be < 2^31");
  }
  embed_bwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_embed_bwd");
}

int mmu_image_normalize(const uint8_t* in, int64_t n, const float* mean, const float* stdv, void* out,
                        int out_dtype, mmu_stream_t stream) {
  if (!in || !out || !mean || !stdv || n < 0) return fail("mmu_image_normalize: bad args");
  if (out_dtype != MMU_BF16 && out_dtype != MMU_F32) return fail("mmu_image_normalize: bad out_dtype");
  for (int c = 0; c < 3; ++c)
    if (!(stdv[c] > 0.f)) return fail("mmu_image_normalize: std must be > 0");
  if (n == 0) return 0;
  image_normalize_launch(in, n, mean, stdv, out, out_dtype == MMU_BF16, (hipStream_t)stream);
  return check_launch("mmu_image_normalize");
}

int mmu_maxpool_fwd(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* y, uint8_t* argmax,
                    mmu_stream_t stream) {
  if (!x || !y || !argmax || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || H > 65536 || W > 65536)
    return fail("mmu_maxpool_fwd: bad args");
  if (off16(x) || off16(y) || off16(argmax)) return fail("mmu_maxpool_fwd: x, y and argmax must be 16-B aligned");
  maxpool3s2_fwd_launch((const bf16*)x, B, (int)H, (int)W, (int)C, (int)((H - 1) / 2 + 1), (int)((W - 1) / 2 + 1),
                        (bf16*)y, argmax, (hipStream_t)stream);
  return check_launch("mmu_maxpool_fwd");
}

int mmu_maxpool_bwd(const void* dy, const uint8_t* argmax, int64_t B, int64_t H, int64_t W, int64_t C, void* dx,
                    mmu_stream_t stream) {
  if (!dy || !dx || !argmax || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || H > 65536 || W > 65536)
    return fail("mmu_maxpool_bwd: bad args");
  if (off16(dy) || off16(dx) || off16(argmax)) return fail("mmu_maxpool_bwd: dy, dx and argmax must be 16-B aligned");
  maxpool3s2_bwd_launch((const bf16*)dy, argmax, B, (int)H, (int)W, (int)C, (int)((H - 1) / 2 + 1),
                        (int)((W - 1) / 2 + 1), (bf16*)dx, (hipStream_t)stream);
  return check_launch("mmu_maxpool_bwd");
}

int mmu_row_pool_fwd(const void* fmap, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n, float* out,
                     mmu_stream_t stream) {
  if (!fmap || !out || C % 8 || n <= 0 || n > Hh) return fail("mmu_row_pool_fwd: bad args");
  if (off16(fmap) || off16(out)) return fail("mmu_row_pool_fwd: fmap and out must be 16-B aligned");
  row_pool_fwd_launch((const bf16*)fmap, B, Hh, Ww, C, n, out, (hipStream_t)stream);
  return check_launch("mmu_row_pool_fwd");
}

int mmu_row_pool_bwd(const float* dout, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n, void* dfmap,
                     mmu_stream_t stream) {
  if (!dout || !dfmap || C % 8 || n <= 0 || n > Hh) return fail("mmu_row_pool_bwd: bad args");
  if (off16(dout) || off16(dfmap)) return fail("mmu_row_pool_bwd: dout and dfmap must be 16-B aligned");
  row_pool_bwd_launch(dout, B, Hh, Ww, C, n, (bf16*)dfmap, (hipStream_t)stream);
  return check_launch("mmu_row_pool_bwd");
}

// the gathered conv products' kernel parameters from their plan (plan.h): ksize 3 (pad 1) or 1 (pad 0)
static void conv_params(GemmParams& p, const ConvShape& c, const ConvPlan& pl, float* ws) {
  p.conv_h = (int)c.H; p.conv_w = (int)c.W; p.conv_c = (int)c.C;
  p.conv_ho = (int)pl.Ho; p.conv_wo = (int)pl.Wo;
  p.conv_ks = (int)c.ksize; p.conv_s = (int)c.stride; p.conv_pad = (int)(c.ksize / 2);
  p.conv_in_bytes = pl.in_bytes;
  p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n;
  p.group_m = 1;
  p.splitk = pl.splitk;
  p.kchunk = pl.kchunk;
  if (pl.splitk > 1) p.ws = ws;
}

int mmu_conv_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W, int64_t Cin,
                   int64_t Cout, int64_t ksize, int64_t stride, int accumulate, float* ws, int64_t ws_floats,
                   mmu_stream_t stream) {
  if (!dY || !X || !dW) return fail("mmu_conv_wgrad: null pointer");
  if (off16(dY) || off16(X) || off16(dW) || off16(ws))
    return fail("mmu_conv_wgrad: dY, X, dW and the workspace must be 16-B aligned");
  const ConvShape c{n_img, H, W, Cin, Cout, ksize, stride, ws ? ws_floats : 0};
  ConvPlan pl;
  if (const char* no = conv_wgrad_plan(c, pl)) return refused(no, pl.why);
  const int64_t T = ksize * ksize;
  GemmParams p{};
  p.A = (const bf16*)dY; p.lda = Cout;  // A = dY^T: M-major [K out pixels][Cout]
  p.B = (const bf16*)X; p.ldb = Cin;    // B gathered: [K out pixels][T Cin]
  p.C = dW; p.ldc = T * Cin;            // dW [Cout][ks][ks][Cin] f32 (channels-last filter)
  p.M = Cout; p.N = T * Cin; p.K = pl.K;
  p.kind = MMU_EPI_STORE;
  p.accumulate = accumulate;
  conv_params(p, c, pl, ws);
  conv3x3_wgrad_launch(p, (hipStream_t)stream);
  return check_launch("mmu_conv_wgrad");
}

int mmu_conv_wgrad_plan(int64_t n_img, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t ksize,
                        int64_t stride, int64_t ws_floats, int64_t* plan) {
  if (!plan) return fail("mmu_conv_wgrad_plan: null plan");
  ConvPlan pl;
  if (const char* no = conv_wgrad_plan(ConvShape{n_img, H, W, Cin, Cout, ksize, stride, ws_floats}, pl))
    return refused(no, pl.why);
  const int64_t out[MMU_CONV_WGRAD_PLAN_FIELDS] = {pl.K,       pl.Ho,  pl.Wo,     pl.tiles_m,
                                                   pl.tiles_n, pl.few, pl.splitk, pl.kchunk};
  for (int i = 0; i < MMU_CONV_WGRAD_PLAN_FIELDS; ++i) plan[i] = out[i];
  return 0;
}

int mmu_conv3x3_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W, int64_t Cin,
                      int64_t Cout, int accumulate, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  return mmu_conv_wgrad(dY, X, dW, n_img, H, W, Cin, Cout, 3, 1, accumulate, ws, ws_floats, stream);
}

static int stem_params(StemParams& p, int64_t n_img, int64_t H, int64_t W, const char* who) {
  if (n_img <= 0 || H < 1 || W < 1 || n_img * H * W * 3 >= (1ll << 31) || n_img > (1 << 20))
    return fail("%s: bad image batch %ld x %ld x %ld", who, n_img, H, W);
  p.n = (int)n_img; p.H = (int)H; p.W = (int)W;
  stem_fill_geometry(p);
  if ((int64_t)p.n * p.Ho * p.Wo * 64 >= (1ll << 31)) return fail("%s: output too large", who);
  return 0;
}

int mmu_stem_conv_fwd(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W,
                      mmu_stream_t stream) {
  if (!X || !Wk || !Y) return fail("mmu_stem_conv_fwd: null pointer");
  if (off16(X) || off16(Wk) || off16(Y)) return fail("mmu_stem_conv_fwd: X, Wk and Y must be 16-B aligned");
  StemParams p{};
  if (stem_params(p, n_img, H, W, "mmu_stem_conv_fwd")) return 1;
  p.X = (const bf16*)X; p.Wt = (const bf16*)Wk; p.Y = (bf16*)Y;
  stem_fwd_launch(p, (hipStream_t)stream);
  return check_launch("mmu_stem_conv_fwd");
}

int64_t mmu_stem_conv_wgrad_ws_floats(int64_t n_img, int64_t H, int64_t W) {
  StemParams p{};
  if (stem_params(p, n_img, H, W, "mmu_stem_conv_wgrad_ws_floats")) return -1;
  return stem_wgrad_ws_floats(p.n_tiles);
}

int mmu_stem_conv_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W,
                        int accumulate, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  if (!dY || !X || !dW || !ws) return fail("mmu_stem_conv_wgrad: null pointer");
  if (off16(dY) || off16(X) || off16(dW) || off16(ws))
    return fail("mmu_stem_conv_wgrad: dY, X, dW and the workspace must be 16-B aligned");
  StemParams p{};
  if (stem_params(p, n_img, H, W, "mmu_stem_conv_wgrad")) return 1;
  if (ws_floats < stem_wgrad_ws_floats(p.n_tiles))
    return fail("mmu_stem_conv_wgrad: ws needs %ld floats", stem_wgrad_ws_floats(p.n_tiles));
  p.X = (const bf16*)X; p.dY = (const bf16*)dY;
  stem_wgrad_launch(p, dW, accumulate, ws, (hipStream_t)stream);
  return check_launch("mmu_stem_conv_wgrad");
}

static int conv_implicit(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                         int64_t N, int64_t ksize, int64_t stride, float* stats, float* ws, int64_t ws_floats,
                         mmu_stream_t stream, const void* bn_x = nullptr, const uint8_t* bn_mask = nullptr,
                         const float* bn_mean = nullptr) {
  if (!X || !Wk || !Y) return fail("mmu_conv_implicit: null pointer");
  // (bn_mask is read by the byte)
  if (off16(X) || off16(Wk) || off16(Y) || off16(stats) || off16(ws) || off16(bn_x) || off16(bn_mean))
    return fail("mmu_conv_implicit: X, Wk, Y, the table, the workspace, bn_x and bn_mean must be 16-B aligned");
  const ConvShape c{n_img, H, W, C, N, ksize, stride, ws ? ws_floats : 0};
  ConvPlan pl;
  if (const char* no = conv_implicit_plan(c, pl)) return refused(no, pl.why);
  const int64_t T = ksize * ksize;
  GemmParams p{};
  p.A = (const bf16*)X; p.lda = C;       // A gathered: [M out pixels][T C]
  p.B = (const bf16*)Wk; p.ldb = T * C;  // B K-major [N][T C]
  p.C = Y; p.ldc = N;                    // Y [M pixels][N] bf16
  p.M = pl.pixels; p.N = N; p.K = pl.K;
  p.kind = !stats ? MMU_EPI_STORE : bn_x ? MMU_EPI_STORE_BNB : MMU_EPI_STORE_STATS;
  p.colsum = stats;
  p.bn_x = (const bf16*)bn_x; p.bn_mask = bn_mask; p.bn_mean = bn_mean;
  conv_params(p, c, pl, ws);
  conv3x3_implicit_launch(p, pl.small, (hipStream_t)stream);
  return check_launch("mmu_conv_implicit");
}

int mmu_conv_implicit_plan(int64_t n_img, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ksize, int64_t stride,
                           int64_t ws_floats, int64_t* plan) {
  if (!plan) return fail("mmu_conv_implicit_plan: null plan");
  ConvPlan pl;
  if (const char* no = conv_implicit_plan(ConvShape{n_img, H, W, C, N, ksize, stride, ws_floats}, pl))
    return refused(no, pl.why);
  const int64_t out[MMU_CONV_IMPLICIT_PLAN_FIELDS] = {pl.small,   pl.pixels, pl.K,      pl.Ho, pl.Wo,
                                                      pl.tiles_m, pl.tiles_n, pl.splitk, pl.kchunk};
  for (int i = 0; i < MMU_CONV_IMPLICIT_PLAN_FIELDS; ++i) plan[i] = out[i];
  return 0;
}

int mmu_conv_implicit(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                      int64_t N, int64_t ksize, int64_t stride, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  return conv_implicit(X, Wk, Y, n_img, H, W, C, N, ksize, stride, nullptr, ws, ws_floats, stream);
}

int mmu_conv_implicit_stats(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                            int64_t N, int64_t ksize, int64_t stride, float* stats, float* ws, int64_t ws_floats,
                            mmu_stream_t stream) {
  if (!stats) return fail("mmu_conv_implicit_stats: null stats table");
  return conv_implicit(X, Wk, Y, n_img, H, W, C, N, ksize, stride, stats, ws, ws_floats, stream);
}

int mmu_conv3x3_implicit(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                         int64_t N, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  return conv_implicit(X, Wk, Y, n_img, H, W, C, N, 3, 1, nullptr, ws, ws_floats, stream);
}

int mmu_conv3x3_implicit_bnb(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                             int64_t N, const void* bn_x, const uint8_t* bn_mask, const float* bn_mean,
                             float* stats, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  if (!stats || !bn_x || !bn_mean) return fail("mmu_conv3x3_implicit_bnb: null table / bn_x / bn_mean");
  return conv_implicit(X, Wk, Y, n_img, H, W, C, N, 3, 1, stats, ws, ws_floats, stream, bn_x, bn_mask, bn_mean);
}

int64_t mmu_batchnorm_ws_bytes(int64_t C) { return batchnorm_ws_bytes(C); }

static int bn_shape(int64_t rows, int64_t C, const char* who) {
  if (rows <= 0 || C <= 0 || C % 8 || C > 2048) return fail("%s: C=%ld must be a multiple of 8, <= 2048", who, C);
  return 0;
}

int mmu_batchnorm_plan(int64_t rows, int64_t C, int64_t* plan) {
  if (!plan) return fail("mmu_batchnorm_plan: null plan");
  if (bn_shape(rows, C, "mmu_batchnorm_plan")) return 1;
  batchnorm_plan(rows, C, plan);
  return 0;
}

static int bn_common(int64_t rows, int64_t C, void* ws, int64_t ws_bytes, const char* who) {
  if (bn_shape(rows, C, who)) return 1;
  if (!ws || ws_bytes < batchnorm_ws_bytes(C) || ((uintptr_t)ws & 15))
    return fail("%s: ws must be >= mmu_batchnorm_ws_bytes(C) bytes, 16-B aligned", who);
  return 0;
}

// the residual stream's residue (y_res / skip_res): the block output (skip + ReLU, the skip's
// residue read) or the downsample's BatchNorm (no skip, no ReLU)
static int bn_res_check(const void* skip, int relu, const void* relu_mask, const void* skip_res, const void* y_res,
                        const char* who) {
  if (skip_res && !y_res) return fail("%s: skip_res needs y_res", who);
  if (!y_res) return 0;
  if (skip && (!relu || !skip_res)) return fail("%s: y_res with a skip needs relu and skip_res", who);
  if (!skip && (relu || relu_mask)) return fail("%s: y_res without a skip takes no relu", who);
  return 0;
}

int mmu_batchnorm_fwd(const void* X, const void* skip, void* Y, int64_t rows, int64_t C, const float* weight,
                      const float* bias, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      int training, float momentum, float eps, int relu, float* save_mean, float* save_invstd,
                      void* relu_mask, const void* skip_res, void* y_res, void* ws, int64_t ws_bytes,
                      mmu_stream_t stream) {
  if (!X || !Y) return fail("mmu_batchnorm_fwd: null pointer");
  if (relu_mask && !relu) return fail("mmu_batchnorm_fwd: relu_mask needs relu");
  if (bn_res_check(skip, relu, relu_mask, skip_res, y_res, "mmu_batchnorm_fwd")) return 1;
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_fwd")) return 1;
  if ((running_mean == nullptr) != (running_var == nullptr))
    return fail("mmu_batchnorm_fwd: running_mean / running_var must both be given or NULL");
  if ((save_mean == nullptr) != (save_invstd == nullptr))
    return fail("mmu_batchnorm_fwd: save_mean / save_invstd must both be given or NULL");
  if (training && rows < 2) return fail("mmu_batchnorm_fwd: training needs more than 1 value per channel");
  if (!training && !running_mean) return fail("mmu_batchnorm_fwd: eval needs running statistics");
  if (training && momentum < 0.f && !num_batches_tracked)
    return fail("mmu_batchnorm_fwd: momentum < 0 (cumulative average) needs num_batches_tracked");
  BnFwdParams q{};
  q.X = (const bf16*)X; q.skip = (const bf16*)skip; q.Y = (bf16*)Y; q.rows = rows; q.C = (int)C;
  q.w = weight; q.b = bias; q.rmean = running_mean; q.rvar = running_var; q.nbt = num_batches_tracked;
  q.training = training; q.relu = relu; q.momentum = momentum; q.eps = eps;
  q.smean = save_mean; q.sinvstd = save_invstd; q.ws = ws; q.mask = (uint8_t*)relu_mask;
  q.skip_res = (const int8_t*)skip_res; q.y_res = (int8_t*)y_res;
  batchnorm_fwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_fwd");
}

int mmu_batchnorm_bwd(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows, int64_t C,
                      const float* weight, const float* save_mean, const float* save_invstd, int relu, void* dX,
                      void* dSkip, float* dweight, float* dbias, void* ws, int64_t ws_bytes, mmu_stream_t stream) {
  if (!dY || !X || !dX || !save_mean || !save_invstd) return fail("mmu_batchnorm_bwd: null pointer");
  if (relu && !Y && !relu_mask) return fail("mmu_batchnorm_bwd: relu needs the forward output Y or its relu_mask");
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_bwd")) return 1;
  BnBwdParams q{};
  q.dY = (const bf16*)dY; q.Y = (const bf16*)Y; q.X = (const bf16*)X; q.rows = rows; q.C = (int)C; q.w = weight;
  q.smean = save_mean; q.sinvstd = save_invstd; q.relu = relu; q.dX = (bf16*)dX; q.dS = (bf16*)dSkip;
  q.dw = dweight; q.db = dbias; q.ws = ws; q.mask = (const uint8_t*)relu_mask;
  batchnorm_bwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_bwd");
}

int mmu_batchnorm_bwd_parts(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                            int64_t C, const float* parts, int64_t nparts, const float* weight,
                            const float* save_mean, const float* save_invstd, int relu, void* dX, void* dSkip,
                            float* dweight, float* dbias, void* ws, int64_t ws_bytes, mmu_stream_t stream) {
  if (!dY || !X || !dX || !save_mean || !save_invstd || !parts || nparts <= 0)
    return fail("mmu_batchnorm_bwd_parts: null pointer / no partials");
  if (relu && !Y && !relu_mask) return fail("mmu_batchnorm_bwd_parts: relu needs the forward output Y or its relu_mask");
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_bwd_parts")) return 1;
  BnBwdParams q{};
  q.dY = (const bf16*)dY; q.Y = (const bf16*)Y; q.X = (const bf16*)X; q.rows = rows; q.C = (int)C; q.w = weight;
  q.smean = save_mean; q.sinvstd = save_invstd; q.relu = relu; q.dX = (bf16*)dX; q.dS = (bf16*)dSkip;
  q.dw = dweight; q.db = dbias; q.ws = ws; q.mask = (const uint8_t*)relu_mask;
  q.parts = parts; q.nparts = nparts;
  batchnorm_bwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_bwd_parts");
}

int mmu_batchnorm_stats(const void* X, int64_t rows, int64_t C, double* sums, void* ws, int64_t ws_bytes,
                        mmu_stream_t stream) {
  if (!X || !sums) return fail("mmu_batchnorm_stats: null pointer");
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_stats")) return 1;
  BnFwdParams q{};
  q.X = (const bf16*)X; q.rows = rows; q.C = (int)C; q.training = 1; q.ws = ws; q.lsum = sums;
  batchnorm_fwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_stats");
}

int mmu_batchnorm_fwd_sums(const void* X, const void* skip, void* Y, int64_t rows, int64_t C, const double* sums,
                           const float* weight, const float* bias, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps, int relu, float* save_mean,
                           float* save_invstd, void* relu_mask, const void* skip_res, void* y_res, void* ws,
                           int64_t ws_bytes, mmu_stream_t stream) {
  if (!X || !Y || !sums) return fail("mmu_batchnorm_fwd_sums: null pointer");
  if (relu_mask && !relu) return fail("mmu_batchnorm_fwd_sums: relu_mask needs relu");
  if (bn_res_check(skip, relu, relu_mask, skip_res, y_res, "mmu_batchnorm_fwd_sums")) return 1;
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_fwd_sums")) return 1;
  if ((running_mean == nullptr) != (running_var == nullptr))
    return fail("mmu_batchnorm_fwd_sums: running_mean / running_var must both be given or NULL");
  if ((save_mean == nullptr) != (save_invstd == nullptr))
    return fail("mmu_batchnorm_fwd_sums: save_mean / save_invstd must both be given or NULL");
  if (momentum < 0.f && !num_batches_tracked)
    return fail("mmu_batchnorm_fwd_sums: momentum < 0 (cumulative average) needs num_batches_tracked");
  BnFwdParams q{};
  q.X = (const bf16*)X; q.skip = (const bf16*)skip; q.Y = (bf16*)Y; q.rows = rows; q.C = (int)C;
  q.w = weight; q.b = bias; q.rmean = running_mean; q.rvar = running_var; q.nbt = num_batches_tracked;
  q.training = 1; q.relu = relu; q.momentum = momentum; q.eps = eps;
  q.smean = save_mean; q.sinvstd = save_invstd; q.ws = ws; q.mask = (uint8_t*)relu_mask; q.gsum = sums;
  q.skip_res = (const int8_t*)skip_res; q.y_res = (int8_t*)y_res;
  batchnorm_fwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_fwd_sums");
}

int mmu_batchnorm_fwd_parts(const void* X, const void* skip, void* Y, int64_t rows, int64_t C, const float* parts,
                            int64_t nparts, const float* weight, const float* bias, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu,
                            float* save_mean, float* save_invstd, void* relu_mask, const void* skip_res, void* y_res,
                            void* ws, int64_t ws_bytes, mmu_stream_t stream) {
  if (!X || !Y || !parts || nparts <= 0) return fail("mmu_batchnorm_fwd_parts: null pointer / no partials");
  if (relu_mask && !relu) return fail("mmu_batchnorm_fwd_parts: relu_mask needs relu");
  if (bn_res_check(skip, relu, relu_mask, skip_res, y_res, "mmu_batchnorm_fwd_parts")) return 1;
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_fwd_parts")) return 1;
  if ((running_mean == nullptr) != (running_var == nullptr))
    return fail("mmu_batchnorm_fwd_parts: running_mean / running_var must both be given or NULL");
  if ((save_mean == nullptr) != (save_invstd == nullptr))
    return fail("mmu_batchnorm_fwd_parts: save_mean / save_invstd must both be given or NULL");
  if (rows < 2) return fail("mmu_batchnorm_fwd_parts: training needs more than 1 value per channel");
  if (momentum < 0.f && !num_batches_tracked)
    return fail("mmu_batchnorm_fwd_parts: momentum < 0 (cumulative average) needs num_batches_tracked");
  BnFwdParams q{};
  q.X = (const bf16*)X; q.skip = (const bf16*)skip; q.Y = (bf16*)Y; q.rows = rows; q.C = (int)C;
  q.w = weight; q.b = bias; q.rmean = running_mean; q.rvar = running_var; q.nbt = num_batches_tracked;
  q.training = 1; q.relu = relu; q.momentum = momentum; q.eps = eps;
  q.smean = save_mean; q.sinvstd = save_invstd; q.ws = ws; q.mask = (uint8_t*)relu_mask;
  q.skip_res = (const int8_t*)skip_res; q.y_res = (int8_t*)y_res;
  q.parts = parts; q.nparts = nparts;
  batchnorm_fwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_fwd_parts");
}

int mmu_batchnorm_bwd_reduce(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                             int64_t C, const float* save_mean, const float* save_invstd, int relu, double* sums,
                             float* dweight, float* dbias, void* ws, int64_t ws_bytes, mmu_stream_t stream) {
  if (!dY || !X || !sums || !save_mean || !save_invstd) return fail("mmu_batchnorm_bwd_reduce: null pointer");
  if (relu && !Y && !relu_mask) return fail("mmu_batchnorm_bwd_reduce: relu needs the forward output Y or its relu_mask");
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_bwd_reduce")) return 1;
  BnBwdParams q{};
  q.dY = (const bf16*)dY; q.Y = (const bf16*)Y; q.X = (const bf16*)X; q.rows = rows; q.C = (int)C;
  q.smean = save_mean; q.sinvstd = save_invstd; q.relu = relu; q.dw = dweight; q.db = dbias; q.ws = ws;
  q.mask = (const uint8_t*)relu_mask; q.lsum = sums;
  batchnorm_bwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_bwd_reduce");
}

int mmu_batchnorm_bwd_sums(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                           int64_t C, const double* sums, const float* weight, const float* save_mean,
                           const float* save_invstd, int relu, void* dX, void* dSkip, void* ws, int64_t ws_bytes,
                           mmu_stream_t stream) {
  if (!dY || !X || !dX || !sums || !save_mean || !save_invstd) return fail("mmu_batchnorm_bwd_sums: null pointer");
  if (relu && !Y && !relu_mask) return fail("mmu_batchnorm_bwd_sums: relu needs the forward output Y or its relu_mask");
  if (bn_common(rows, C, ws, ws_bytes, "mmu_batchnorm_bwd_sums")) return 1;
  BnBwdParams q{};
  q.dY = (const bf16*)dY; q.Y = (const bf16*)Y; q.X = (const bf16*)X; q.rows = rows; q.C = (int)C; q.w = weight;
  q.smean = save_mean; q.sinvstd = save_invstd; q.relu = relu; q.dX = (bf16*)dX; q.dS = (bf16*)dSkip; q.ws = ws;
  q.mask = (const uint8_t*)relu_mask; q.gsum = sums;
  batchnorm_bwd_launch(q, (hipStream_t)stream);
  return check_launch("mmu_batchnorm_bwd_sums");
}

int mmu_bertadam_step(float* params, const float* grads, float* m, float* v, void* bf16_copy, const int64_t* table,
                      int32_t* steps, int64_t n_tensors, int64_t n_chunks, float lr_decay, float lr_nodecay, float wd,
                      float warmup, float t_total, float b1, float b2, float eps, float max_grad_norm,
                      float grad_scale, float* ws, int64_t ws_floats, mmu_stream_t stream) {
  if (!params || !grads || !m || !v || !table || !steps || !ws) return fail("mmu_bertadam_step: null pointer");
  if (n_tensors <= 0 || n_chunks <= 0) return fail("mmu_bertadam_step: empty table");
  if (ws_floats < n_chunks + 2 * n_tensors) return fail("mmu_bertadam_step: workspace too small");
  if (!(grad_scale > 0.f)) return fail("mmu_bertadam_step: grad_scale must be > 0");
  AdamParams p{};
  p.params = params; p.grads = grads; p.m = m; p.v = v; p.bf16_copy = (bf16*)bf16_copy; p.table = table;
  p.steps = steps; p.n_tensors = n_tensors; p.total = n_chunks; p.lr_decay = lr_decay; p.lr_nodecay = lr_nodecay;
  p.wd = wd; p.warmup = warmup; p.t_total = t_total; p.b1 = b1; p.b2 = b2; p.eps = eps;
  p.max_grad_norm = max_grad_norm; p.grad_scale = grad_scale; p.ws = ws; p.ws_floats = ws_floats;
  const char* e = nullptr;
  if (bertadam_launch(p, (hipStream_t)stream, &e)) return fail("mmu_bertadam_step: %s", e ? e : "failed");
  return check_launch("mmu_bertadam_step");
}

int mmu_uncertainty(const float* logits, const int64_t* y, int64_t S, int64_t R, int64_t C, float* p_bar, float* nll,
                    float* conf, float* correct, mmu_stream_t stream) {
  if (!logits || !y || !p_bar || !nll || !conf || !correct) return fail("mmu_uncertainty: null pointer");
  if (S <= 0 || R <= 0 || C <= 0 || C > 1024) return fail("mmu_uncertainty: bad shape (C <= 1024)");
  uncertainty_launch(logits, y, S, R, C, p_bar, nll, conf, correct, (hipStream_t)stream);
  return check_launch("mmu_uncertainty");
}

int mmu_ece_bins(const float* conf, const float* correct, int64_t S, int64_t n_bins, float* out, mmu_stream_t stream) {
  if (!conf || !correct || !out || S <= 0 || n_bins <= 0) return fail("mmu_ece_bins: bad args");
  ece_bins_launch(conf, correct, S, n_bins, out, (hipStream_t)stream);
  return check_launch("mmu_ece_bins");
}

// ---------------------------------------------------------------- the ensemble-statistics entries
struct StackPtr { const char* name; const void* p; };
struct StackExtent { const char* name; int64_t v; };
struct StackAxis { const char* name; int64_t stride, extent; };
struct StackRange { bool bad; const char* fmt; int64_t v; };  // an entry's own range check; fmt takes who and v

// element strides of a logit stack with a contiguous class axis: the axes that step (extent > 1), by
// ascending stride, must each clear the span of the one below it
static int check_skt_strides(const char* who, const StackAxis (&axes)[3], int64_t C) {
  StackAxis ax[3] = {axes[0], axes[1], axes[2]};
  for (int i = 1; i < 3; ++i)
    for (int j = i; j > 0 && ax[j].stride < ax[j - 1].stride; --j) std::swap(ax[j], ax[j - 1]);
  int64_t span = C;
  const char* below = "C";
  for (const StackAxis& a : ax) {
    if (a.extent == 1) continue;
    if (a.stride < span)
      return fail("%s: %s = %lld is smaller than the %lld elements the %s axis below it spans (overlapping layout)",
                  who, a.name, (long long)a.stride, (long long)span, below);
    if (a.stride > INT64_MAX / a.extent) return fail("%s: %s = %lld overflows", who, a.name, (long long)a.stride);
    span = a.stride * a.extent;
    below = a.name;
  }
  return 0;
}

// The refusals of every entry that reads a logit stack, in the order each of them reports: a null
// pointer, an extent that is not positive, the entry's range checks that come before the class limit,
// C > 1024, its other range checks, the grid limit of S (the extent of axes[0]), the strides.
static int stack_check(const char* who, std::initializer_list<StackPtr> ptrs,
                       std::initializer_list<StackExtent> extents, int64_t C,
                       std::initializer_list<StackRange> before_classes,
                       std::initializer_list<StackRange> after_classes, const StackAxis (&axes)[3]) {
  for (const StackPtr& a : ptrs)
    if (!a.p) return fail("%s: %s is null", who, a.name);
  for (const StackExtent& e : extents)
    if (e.v <= 0) return fail("%s: %s = %lld must be positive", who, e.name, (long long)e.v);
  for (const StackRange& r : before_classes)
    if (r.bad) return fail(r.fmt, who, (long long)r.v);
  if (C > 1024) return fail("%s: C = %lld exceeds 1024 classes", who, (long long)C);
  for (const StackRange& r : after_classes)
    if (r.bad) return fail(r.fmt, who, (long long)r.v);
  const int64_t S = axes[0].extent;
  if (S > 0x7fffffffLL) return fail("%s: S = %lld exceeds the grid limit 2147483647", who, (long long)S);
  return check_skt_strides(who, axes, C);
}

// mmu_uncertainty_decompose and mmu_uncertainty_decompose_scaled
static int decompose_check(const char* who, const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                           int64_t S, int64_t K, int64_t T, int64_t C, float* stats, float* p_bar) {
  return stack_check(who, {{"logits", logits}, {"y", y}, {"stats", stats}, {"p_bar", p_bar}},
                     {{"S", S}, {"K", K}, {"T", T}, {"C", C}}, C, {}, {},
                     {{"ss", ss, S}, {"sk", sk, K}, {"st", st, T}});
}

int mmu_uncertainty_decompose(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                              int64_t K, int64_t T, int64_t C, float* stats, float* p_bar, float* member_nll,
                              mmu_stream_t stream) {
  const char* who = "mmu_uncertainty_decompose";
  if (decompose_check(who, logits, ss, sk, st, y, S, K, T, C, stats, p_bar)) return 1;
  uncertainty_decompose_launch(logits, ss, sk, st, y, S, K, T, C, stats, p_bar, member_nll, nullptr,
                               (hipStream_t)stream);
  return check_launch(who);
}

int mmu_uncertainty_decompose_scaled(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                                     int64_t S, int64_t K, int64_t T, int64_t C, float* stats, float* p_bar,
                                     float* member_nll, const float* inv_temp, mmu_stream_t stream) {
  const char* who = "mmu_uncertainty_decompose_scaled";
  if (decompose_check(who, logits, ss, sk, st, y, S, K, T, C, stats, p_bar)) return 1;
  uncertainty_decompose_launch(logits, ss, sk, st, y, S, K, T, C, stats, p_bar, member_nll, inv_temp,
                               (hipStream_t)stream);
  return check_launch(who);
}

int mmu_temperature_nll(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                        int64_t K, int64_t T, int64_t C, const float* inv_temp, int64_t J, float* nll,
                        double* nll_sum, mmu_stream_t stream) {
  const char* who = "mmu_temperature_nll";
  if (stack_check(who, {{"logits", logits}, {"y", y}, {"inv_temp", inv_temp}, {"nll", nll}},
                  {{"S", S}, {"K", K}, {"T", T}, {"C", C}, {"J", J}}, C, {},
                  {{J > 64, "%s: J = %lld exceeds 64 candidates", J}}, {{"ss", ss, S}, {"sk", sk, K}, {"st", st, T}}))
    return 1;
  temperature_nll_launch(logits, ss, sk, st, y, S, K, T, C, inv_temp, J, nll, nll_sum, (hipStream_t)stream);
  return check_launch(who);
}

int mmu_robustness_summary(const float* logits, int64_t ss, int64_t sv, int64_t sk, const int64_t* y, int64_t S,
                           int64_t V, int64_t K, int64_t C, float* stats, float* per_variant, mmu_stream_t stream) {
  const char* who = "mmu_robustness_summary";
  if (stack_check(who, {{"logits", logits}, {"y", y}, {"stats", stats}}, {{"S", S}, {"K", K}, {"C", C}}, C,
                  {{V < 5, "%s: V = %lld is fewer than the 5 variants of one control repeat (V = 3 + 2n)", V},
                   {V % 2 == 0, "%s: V = %lld must be odd (V = 3 + 2n)", V},
                   {V > 1023, "%s: V = %lld exceeds 1023 variants", V}},
                  {}, {{"ss", ss, S}, {"sv", sv, V}, {"sk", sk, K}}))
    return 1;
  robustness_summary_launch(logits, ss, sv, sk, y, S, V, K, C, stats, per_variant, (hipStream_t)stream);
  return check_launch(who);
}

int mmu_ensemble_diversity(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                           int64_t K, int64_t T, int64_t C, int64_t top, int mute_true, float* pair, int32_t* counts,
                           int32_t* member_arg, mmu_stream_t stream) {
  const char* who = "mmu_ensemble_diversity";
  if (stack_check(who, {{"logits", logits}, {"y", y}, {"pair", pair}, {"member_arg", member_arg}},
                  {{"S", S}, {"T", T}, {"C", C}}, C, {},
                  {{K < 2, "%s: K = %lld is fewer than the 2 members of one pair", K},
                   {K > 16, "%s: K = %lld exceeds 16 members", K},
                   {top < 0, "%s: top = %lld must not be negative (0: no truncation)", top},
                   {top > 1024, "%s: top = %lld exceeds 1024", top},
                   {mute_true != 0 && mute_true != 1, "%s: mute_true = %lld must be 0 or 1", mute_true}},
                  {{"ss", ss, S}, {"sk", sk, K}, {"st", st, T}}))
    return 1;
  const hipError_t e = ensemble_diversity_launch(logits, ss, sk, st, y, S, K, T, C, top, mute_true, pair, counts,
                                                 member_arg, (hipStream_t)stream);
  if (e != hipSuccess) return fail("%s: the LDS request was refused: %s", who, hipGetErrorString(e));
  return check_launch(who);
}

int mmu_rank_table(const float* x, int64_t ss, int64_t sj, const uint8_t* group, int64_t S, int64_t J, int32_t* rank,
                   int64_t* counts, mmu_stream_t stream) {
  const char* who = "mmu_rank_table";
  if (!x) return fail("%s: x is null", who);
  if (!group) return fail("%s: group is null", who);
  if (!counts) return fail("%s: counts is null", who);
  if (S <= 0) return fail("%s: S = %lld must be positive", who, (long long)S);
  if (J <= 0) return fail("%s: J = %lld must be positive", who, (long long)J);
  if (S > MMU_RANK_MAX_S)
    return fail("%s: S = %lld exceeds %d samples (the sweep is O(S^2) per column)", who, (long long)S, MMU_RANK_MAX_S);
  if (J > MMU_RANK_MAX_J) return fail("%s: J = %lld exceeds %d columns", who, (long long)J, MMU_RANK_MAX_J);
  // the axes that step (extent > 1): positive strides, and the larger must clear the span of the smaller
  // (the rule of check_skt_strides, over scalars)
  StackAxis lo = {"ss", ss, S}, hi = {"sj", sj, J};
  for (const StackAxis& a : {lo, hi}) {
    if (a.extent == 1) continue;
    if (a.stride <= 0) return fail("%s: %s = %lld must be positive", who, a.name, (long long)a.stride);
    if (a.stride > INT64_MAX / 8 / a.extent) return fail("%s: %s = %lld overflows", who, a.name, (long long)a.stride);
  }
  if (S > 1 && J > 1) {
    if (hi.stride < lo.stride) std::swap(lo, hi);
    if (hi.stride < lo.stride * lo.extent)
      return fail("%s: %s = %lld is smaller than the %lld elements the %s axis below it spans (overlapping layout)",
                  who, hi.name, (long long)hi.stride, (long long)(lo.stride * lo.extent), lo.name);
  }
  if ((uintptr_t)x & 3) return fail("%s: x is not 4-byte aligned", who);
  if ((uintptr_t)rank & 3) return fail("%s: rank is not 4-byte aligned", who);
  if ((uintptr_t)counts & 7) return fail("%s: counts is not 8-byte aligned", who);
  const hipError_t e = rank_table_launch(x, ss, sj, group, S, J, rank, counts, (hipStream_t)stream);
  if (e != hipSuccess) return fail("%s: zeroing counts failed: %s", who, hipGetErrorString(e));
  return check_launch(who);
}

}  // extern "C"
